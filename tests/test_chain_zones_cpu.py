"""The inputs and the algebra of tests/test_chain_selects_gpu.py, on the oracle and NumPy alone (no
GPU): the zone bank reaches every zone of the lean atan (fastmath.hpp atan_zones), the three-zone
formula restated in NumPy is an atan, and the one-select octant fix-up (octant_fix) has the bits of
the select it replaces."""
import numpy as np

import chain_zones as Z


def _arguments():
    """10^6 arguments — uniform over +-4 (all three zones, densely around their edges) and Cauchy
    x 3 (the tails of zone III, tiny values of zone I) — plus the edge list of the device test."""
    rng = np.random.RandomState(5)
    return np.concatenate([rng.uniform(-4, 4, 500000), rng.standard_cauchy(500000) * 3, Z.atan_edges()])


def test_zone_bank_reaches_every_zone():
    """Every zone of atan(B slip) holds at least 5 % of the oracle's stage evaluations of the
    N = 65, C = 3, H = 20 rollouts of the zone bank (measured: 41 / 37 / 22 %), and of the first
    step alone (H = 1: the zones are reached from the start, not only late in the rollout)."""
    x0, _, _ = Z.start()
    for H in (20, 1):
        traj, az = Z.oracle_rollout_recording_atan(Z.zone_bank(), x0, Z.candidates(3, H))
        assert az.size == 2 * 4 * H * 3 * Z.NMAX and np.isfinite(traj).all()
        fr = Z.zone_fractions(az)
        print(f"ZONES H={H}: I {fr[0]:.3f}, II {fr[1]:.3f}, III {fr[2]:.3f} of {az.size} stage evaluations")
        assert min(fr) >= 0.05, fr


def test_three_zone_formula_is_atan():
    """The reduction and the reconstruction of atan_zones with NumPy's own atan of the reduced
    argument: within 2 ulp of numpy.arctan (the pi/4 constant's own error is 0.55 ulp of a result
    below 1/2, the reduced argument carries up to three roundings, the core and the sum one
    each); odd bitwise; +-inf gives +-pi/2 and NaN gives NaN.  With the precise 10-term polynomial
    in place of NumPy's core (no FMAs in NumPy: one rounding more per term) the figure is printed
    and held to the precise cores' 4 ulp."""
    z = _arguments()
    want = np.arctan(z)
    got = Z.atan_three_zone(z)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[np.isinf(z)], np.copysign(Z.PIO2, z[np.isinf(z)]))
    u, up = Z.ulp_err(got, want), Z.ulp_err(Z.atan_three_zone(z, Z.poly10), want)
    print(f"three-zone restatement: {u:.1f} ulp (NumPy core), {up:.1f} ulp (10-term polynomial)")
    assert u <= 2 and up <= 4
    fin = ~np.isnan(z)
    np.testing.assert_array_equal(Z.atan_three_zone(-z[fin]).view(np.int64), (-got[fin]).view(np.int64))


def test_one_select_fixup_has_the_bits_of_the_select():
    """copysign(fma(w, pi/2, -r), y), w = swap ? 1 : 0, against copysign(swap ? pi/2 - r : r, y) on
    the reduced results r of the same arguments (atan: swap = |z| > 1) and on r at its extremes
    (+-0, tiny, pi/4 and its neighbours, NaN) under both values of swap and both signs."""
    z = _arguments()
    swap, r = Z.atan_two_way_parts(z)
    np.testing.assert_array_equal(Z.fixup_fma(swap, r, z).view(np.int64), Z.fixup_select(swap, r, z).view(np.int64))
    r = np.array([0.0, Z.TINY, 1e-300, np.nextafter(Z.PIO4, 0), Z.PIO4, np.nextafter(Z.PIO4, 1), 0.3, np.nan])
    for sw in (False, True):
        for y in (1.0, -1.0):
            a = Z.fixup_fma(np.full(r.shape, sw), r, np.full(r.shape, y))
            b = Z.fixup_select(np.full(r.shape, sw), r, np.full(r.shape, y))
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
            m = ~np.isnan(a)
            np.testing.assert_array_equal(a[m].view(np.int64), b[m].view(np.int64))
