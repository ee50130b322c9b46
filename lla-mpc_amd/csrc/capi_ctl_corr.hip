// capi_ctl_corr.hip — the controller's soft track corridor (llampc_ctl_set_track /
// llampc_ctl_set_corridor; ctl.hpp CtlCorridor): the track tables, the switch, the debug read-backs and
// the corridor tick's variant question.  The corridor's device state is capi_host.hpp ctl_cor_layout's.
#include "capi_ctl.hpp"

using namespace llampc;

extern "C" {

int llampc_ctl_set_track(llampc_ctl* c, const double* centre, const double* theta, int32_t n, double track_length,
                         double track_width) {
  if (!c || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (c->cor_w > 0) return fail(LLAMPC_E_STATE, "switch the corridor off before replacing its track");
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  return c->track.upload(b->stream, centre, theta, n, track_length, track_width);
}

int llampc_ctl_set_corridor(llampc_ctl* c, double weight, double margin) {
  if (!c) return fail(LLAMPC_E_ARG, "controller is NULL");
  std::lock_guard<std::mutex> lc(c->mu);
  if (const char* why = ctl_solver_blocks(c->solver_attached, CtlSetter::corridor, weight > 0)) return fail(LLAMPC_E_STATE, "%s", why);
  ctl_cancel(c);                         // as every other call: the tick after launches normally
  llampc_bank* b = c->b;
  const llampc_ctl_cfg& k = c->cfg;
  const CtlCorridorFacts facts{c->pending, c->mb || c->xg_world, c->no_stage, c->track.n, c->track.width, b->n, k.C, k.H, k.K, b->rl_n};
  char why[256];
  if (int rc = ctl_corridor_refused(facts, weight, margin, why, sizeof why)) return fail(rc, "%s", why);
  if (weight > 0) {
    if (!c->d_cor) {
      constexpr CtlCorLayout Y = ctl_cor_layout();
      DeviceGuard g(b->device);
      DevBuf<double> cor;
      DevBuf<uint64_t> tag;
      DevBuf<int32_t> flag;
      int rc;
      if ((rc = cor.zalloc(Y.cor_doubles, "corridor path state")) || (rc = tag.zalloc(Y.hp_tag_words, "corridor words")) ||
          (rc = flag.zalloc(Y.flags, "corridor flags")))
        return rc;
      c->d_cor = std::move(cor);
      c->d_hp_tag = std::move(tag);
      c->d_cor_flag = std::move(flag);
    }
    if (k.debug_inputs && !c->d_cor_cost) {
      DeviceGuard g(b->device);
      if (int rc = c->d_cor_cost.zalloc((size_t)kCtlSlotsMax * k.C, "corridor costs")) return rc;
    }
  } else {
    c->cor_prev = false;                 // off: the path state is invalid from here on
  }
  c->cor_w = weight;
  c->cor_margin = margin;
  return LLAMPC_OK;
}

int llampc_ctl_corridor(llampc_ctl* c, double* path, double* hp, double* theta, int32_t* valid) {
  if (!c || !path || !hp || !theta || !valid) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!c->d_cor || !c->cor_prev) return fail(LLAMPC_E_STATE, "the last tick was not a corridor tick");
  DeviceGuard g(c->b->device);
  ctl_cancel(c);                         // an armed launch would hold the stream (re-armed next tick)
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  constexpr CtlCorLayout Y = ctl_cor_layout();
  const int H = c->cfg.H;
  const int cp = (int)((c->t - 1) & 1);  // the last tick's copy
  std::vector<double> h(Y.rb_doubles);
  int32_t v = 0;
  HIP_TRY(hipMemcpy(h.data(), c->d_cor.get() + Y.rb(cp), h.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&v, c->d_cor_flag.get() + Y.rb_valid(cp), sizeof v, hipMemcpyDeviceToHost));
  for (int r = 0; r < 2; ++r) std::memcpy(path + (size_t)r * (H + 1), h.data() + (size_t)r * Y.row, (H + 1) * sizeof(double));
  std::memcpy(hp, h.data() + Y.rb_hp, 6 * (size_t)H * sizeof(double));
  std::memcpy(theta, h.data() + Y.rb_theta, (size_t)H * sizeof(double));
  *valid = v;
  return LLAMPC_OK;
}

int llampc_ctl_corridor_costs(llampc_ctl* c, double* costs, int32_t* nslots) {
  if (!c || !costs || !nslots) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!c->d_cor_cost) return fail(LLAMPC_E_STATE, "controller created without debug_inputs");
  if (!c->cor_prev) return fail(LLAMPC_E_STATE, "the last tick was not a corridor tick");
  DeviceGuard g(c->b->device);
  ctl_cancel(c);                         // an armed launch would hold the stream (re-armed next tick)
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  HIP_TRY(hipMemcpy(costs, c->d_cor_cost.get(), (size_t)c->cor_nslots * c->cfg.C * sizeof(double), hipMemcpyDeviceToHost));
  *nslots = c->cor_nslots;
  return LLAMPC_OK;
}

// llampc_ctl_variant's fields for a corridor tick on a centre line of track_n points, then the
// corridor block count: from the same ctl_shape.
int llampc_ctl_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t track_n,
                                int32_t out[10]) {
  CtlShape V{};
  char why[256];
  if (int rc = ctl_variant_refused(!out, n, C, H, K, rl_n, &track_n, false, V, why, sizeof why)) return fail(rc, "%s", why);
  const int32_t v[10] = {V.lpm, V.G, V.cpl, V.mpb, V.s4, V.zfit, V.R, V.nb_lb, V.nb_la, V.nb_cor};
  std::memcpy(out, v, sizeof v);
  return LLAMPC_OK;
}

}  // extern "C"
