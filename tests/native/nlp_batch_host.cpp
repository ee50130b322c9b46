// Host harness for the batched NLP solve's pure host helpers in csrc/capi_host.hpp (test
// infrastructure): the buffer layout, the record pack, the create / solve refusals and the B-tag
// wait, run on the CPU — built with AddressSanitizer and UBSan (host code only), every buffer a
// heap block of exactly the size the layout claims, so a write past a problem's region or past the
// buffer's end is an error here before any GPU is involved.
//   nlp_batch_host layout H samples B      the layout's words, then B packed records read back
//   nlp_batch_host create n samples max_batch cus
//   nlp_batch_host args B max_batch n null_mask idx...   (null_mask bit i: pointer i is NULL)
//   nlp_batch_host tags B want set_mask     B tags, those in set_mask written; a 1 ms bound
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "capi_host.hpp"

using namespace llampc;

static_assert(sizeof(NlpBatch) == 40, "NlpBatch layout");

static int layout(int H, int samples, int B) {
  const NlpBatchLayout l = nlp_batch_layout(H, samples);
  const NlpBatch a = nlp_batch_arg(l, nullptr, samples);
  std::printf("%zu %zu %zu %zu %zu %zu %d\n", l.rec_words, l.up_off, l.list_words, l.cand_doubles, l.ms_words,
              l.tag_words, a.nl_log2);
  if (a.rec_words != l.rec_words || a.up_off != l.up_off || a.list_words != l.list_words ||
      a.cand_doubles != l.cand_doubles || a.ms_words != l.ms_words || a.tag_words != l.tag_words)
    return 4;
  // B records in a block of exactly B rec_words words, packed from inputs of exactly their sizes
  // and read back after all are written: a record that ran into a neighbour shows in either
  std::unique_ptr<uint64_t[]> buf(new uint64_t[(size_t)B * l.rec_words]);
  for (size_t i = 0; i < (size_t)B * l.rec_words; ++i) buf[i] = ~0ull;
  auto val = [](int p, int field, int i) { return 1000.0 * p + 100.0 * field + i; };
  for (int p = B - 1; p >= 0; --p) {
    std::unique_ptr<double[]> x0(new double[6]), xref(new double[2 * (H + 1)]), up(new double[2]),
        base(new double[2 * H]);
    for (int i = 0; i < 6; ++i) x0[i] = val(p, 0, i);
    for (int i = 0; i < 2 * (H + 1); ++i) xref[i] = val(p, 1, i);
    for (int i = 0; i < 2; ++i) up[i] = val(p, 2, i);
    for (int i = 0; i < 2 * H; ++i) base[i] = val(p, 3, i);
    nlp_batch_pack(l, H, buf.get() + p * l.rec_words, x0.get(), xref.get(), up.get(), p % 2 ? base.get() : nullptr,
                   0x100000000ull * p + 7, 3 * p + 1, p % 2);
  }
  for (int p = 0; p < B; ++p) {
    const uint64_t* r = buf.get() + p * l.rec_words;
    const double* d = reinterpret_cast<const double*>(r);
    int bad = 0;
    for (int i = 0; i < 6; ++i) bad += d[i] != val(p, 0, i);
    for (int i = 0; i < 2 * (H + 1); ++i) bad += d[6 + i] != val(p, 1, i);
    for (int i = 0; i < 2 * H; ++i) bad += d[6 + 2 * (H + 1) + i] != (p % 2 ? val(p, 3, i) : val(p, 2, i % 2));
    for (int i = 0; i < 2; ++i) bad += d[l.up_off + i] != val(p, 2, i);
    bad += r[l.up_off + 2] != 0x100000000ull * p + 7;
    bad += (uint32_t)r[l.up_off + 3] != (uint32_t)(3 * p + 1) || (int32_t)(r[l.up_off + 3] >> 32) != p % 2;
    for (size_t i = l.up_off + 4; i < l.rec_words; ++i) bad += r[i] != ~0ull;   // the pad is untouched
    std::printf("%d %d\n", p, bad);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto I = [&](int i) { return std::atoll(argv[i]); };
  if (mode == "layout" && argc == 5) return layout((int)I(2), (int)I(3), (int)I(4));
  if (mode == "create" && argc == 6) {
    const char* why = nlp_batch_create_invalid(I(2), (int32_t)I(3), (int32_t)I(4), (int32_t)I(5));
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (mode == "args" && argc >= 6) {
    const int32_t B = (int32_t)I(2), mb = (int32_t)I(3);
    const int64_t n = I(4);
    const long mask = (long)I(5);
    std::vector<int64_t> idx;
    for (int i = 6; i < argc; ++i) idx.push_back(I(i));
    int dummy = 0;
    auto ptr = [&](int bit) -> const void* { return (mask >> bit) & 1 ? nullptr : &dummy; };
    const char* why = nlp_batch_args_invalid(B, mb, (mask & 1) ? nullptr : idx.data(), n, ptr(1), ptr(2), ptr(3), ptr(4),
                                             ptr(5), ptr(6), ptr(7), ptr(8));
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (mode == "tags" && argc == 5) {
    const int32_t B = (int32_t)I(2);
    const uint64_t want = (uint64_t)I(3);
    const long mask = (long)I(4);
    const size_t stride = nlp_batch_layout(1, 64).tag_words;
    std::unique_ptr<uint64_t[]> tags(new uint64_t[(size_t)B * stride]());
    for (int p = 0; p < B; ++p) tags[p * stride] = (mask >> p) & 1 ? want : want - 1;
    std::unique_ptr<bool[]> arrived(new bool[B]());
    int timeouts = 0;
    const int rc = spin_for_tags(tags.get(), stride, B, want, arrived.get(), [&]() { return ++timeouts, 0; },
                                 std::chrono::milliseconds(1));
    std::printf("%d %d", rc, timeouts);
    for (int p = 0; p < B; ++p) std::printf(" %d", (int)arrived[p]);
    std::printf("\n");
    return 0;
  }
  return 2;
}
