// Stand-alone host check of the teacher cfg decoder (csrc/teacher_cfg.h), meant for a sanitizer build; no HIP, no library:
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/teacher_cfg_check.cpp -o teacher_cfg_check && ./teacher_cfg_check
//
// (the runtimes linked in: the program then runs whatever the environment preloads; tests/test_teacher_cfg_cpu.py runs it.)
// Packs a cfg by the layout INTEGRATION.md documents (written out here a second time, on purpose) for every combination
// of {plain, shared trunk, contacts, only_contact} x {fixed, adaptive} x {stop off, on}, decodes it and compares field by
// field.  Then the decoder gets what it must refuse: every pair of list lengths 0 .. full + 2 that is not itself a valid
// packing, each mode flag at 0 / 2 / -1, ints outside 32 bits at every position, NaN / zero / negative thresholds and
// rates, and a stop tail without a stop record.  A refusal must return IGI_E_BADARG with text; every list is handed over in
// a heap block of exactly its length, so a read past either end is a sanitizer report.
#include <algorithm>
#include <limits>
#include <vector>

#include "../isaacgyminsertion_amd/csrc/teacher_cfg.h"

namespace {
constexpr int M = IGI_MAX_LAYERS;
using Ints = std::vector<int64_t>;
using Floats = std::vector<double>;
long long accepted = 0, refused = 0, bad = 0;

struct Case { int mode, sched, stop; };   // mode: 0 plain, 1 shared, 2 contacts, 3 only_contact
const int64_t DIMS[4] = {15, 64, 6, 3}, PRIV_UNITS[M] = {256, 128, 8, 0}, UNITS[M] = {512, 256, 128, 0}, NTE[3] = {64, 8, 4};
const int64_t CONTACTS[2] = {37, 8};
const double HYPER[12] = {0.99, 0.95, 5e-4, 0.9, 0.999, 1e-8, 0.2, 4.0, 0.001, 1e-4, 1.0, 1e-5}, SCHED[3] = {0.008, 1e-6, 1e-2};

void pack(const Case& k, Ints* ic, Floats* fc) {
  ic->assign(DIMS, DIMS + 4);
  ic->insert(ic->end(), PRIV_UNITS, PRIV_UNITS + M);
  ic->push_back(3);
  ic->insert(ic->end(), UNITS, UNITS + M);
  ic->insert(ic->end(), NTE, NTE + 3);
  if (k.mode == 1) { ic->push_back(1); ic->push_back(0); }
  if (k.mode >= 2) { ic->push_back(CONTACTS[0]); ic->push_back(CONTACTS[1]); ic->push_back(k.mode == 3); }
  fc->assign(HYPER, HYPER + 12);
  if (k.sched) { ic->push_back(1); fc->insert(fc->end(), SCHED, SCHED + 3); }
  if (k.stop) { ic->push_back(1); fc->push_back(SCHED[0]); }
}

// whether lists of these lengths and trailing values are a packing at all, by the documented rule (lengths tell the mode)
bool valid(Ints ic, Floats fc, bool with_stop) {
  if (with_stop && (fc.size() == 13 || fc.size() == 16)) {
    if (ic.empty() || ic.back() != 1 || !(fc.back() > 0)) return false;
    if (fc.size() == 16 && fc.back() != fc[12]) return false;
    ic.pop_back(); fc.pop_back();
  }
  if (fc.size() == 15) {
    if (ic.empty() || ic.back() != 1 || !(fc[12] > 0) || !(fc[13] > 0) || !(fc[13] <= fc[14])) return false;
    ic.pop_back(); fc.resize(12);
  }
  if (fc.size() != 12) return false;
  for (int64_t v : ic) if (v != (int32_t)v) return false;
  if (ic.size() == 10 + 2 * M) return ic[8 + 2 * M] == 1 && ic[9 + 2 * M] == 0;
  if (ic.size() == 11 + 2 * M) return ic[8 + 2 * M] >= 1;
  return ic.size() == 8 + 2 * M;
}

// one call of the decoder on exact-size heap copies; checks the contract of either outcome
int64_t decode(const Ints& ic, const Floats& fc, igi_teacher_cfg* c, igi_kl_stop* ks) {
  int64_t* pi = new int64_t[ic.size()];
  double* pf = new double[fc.size()];
  std::copy(ic.begin(), ic.end(), pi);
  std::copy(fc.begin(), fc.end(), pf);
  char err[256] = "?";
  const int64_t r = igi_teacher_cfg_decode(pi, (int)ic.size(), pf, (int)fc.size(), c, ks, err, sizeof(err));
  delete[] pi;
  delete[] pf;
  if (r >= 0) { ++accepted; if (err[0]) { ++bad; printf("accepted with text: %s\n", err); } }
  else { ++refused; if (r != IGI_E_BADARG || !err[0] || err[0] == '?') { ++bad; printf("refusal %lld without text\n", (long long)r); } }
  return r;
}

void expect(bool accept, const Ints& ic, const Floats& fc, bool with_stop, const char* what) {
  igi_teacher_cfg c;
  igi_kl_stop ks;
  const bool got = decode(ic, fc, &c, with_stop ? &ks : nullptr) >= 0;
  if (got != accept) { ++bad; printf("%s: %zu ints, %zu floats: %s\n", what, ic.size(), fc.size(), got ? "accepted" : "refused"); }
}

void round_trip(const Case& k) {
  Ints ic; Floats fc;
  pack(k, &ic, &fc);
  igi_teacher_cfg c;
  igi_kl_stop ks;
  const int64_t steps = decode(ic, fc, &c, &ks);
  bool ok = steps == (k.stop ? 4 * ((64 * 8) / ((64 * 8) / 4)) : 0);
  ok = ok && c.obs_dim == 15 && c.priv_dim == 64 && c.act_dim == 6 && c.n_priv_layers == 3 && c.n_layers == 3 && c.num_envs == 64 &&
       c.horizon == 8 && c.mini_epochs == 4;
  for (int i = 0; i < M; ++i) ok = ok && c.priv_units[i] == PRIV_UNITS[i] && c.units[i] == UNITS[i];
  ok = ok && c.shared_parameters == (k.mode == 1) && c.contact_points == (k.mode >= 2 ? 37 : 0) &&
       c.contact_emb == (k.mode >= 2 ? 8 : 0) && c.only_contact == (k.mode == 3);
  ok = ok && c.gamma == HYPER[0] && c.tau == HYPER[1] && c.lr == HYPER[2] && c.beta1 == HYPER[3] && c.beta2 == HYPER[4] &&
       c.adam_eps == HYPER[5] && c.e_clip == (float)HYPER[6] && c.critic_coef == (float)HYPER[7] && c.entropy_coef == (float)HYPER[8] &&
       c.bounds_loss_coef == (float)HYPER[9] && c.grad_norm == (float)HYPER[10] && c.rms_eps == (float)HYPER[11];
  ok = ok && c.lr_schedule == k.sched && c.kl_threshold == (k.sched ? SCHED[0] : 0) && c.lr_min == (k.sched ? SCHED[1] : 0) &&
       c.lr_max == (k.sched ? SCHED[2] : 0);
  ok = ok && ks.kl_early_stop == k.stop && ks.kl_threshold == (k.stop ? SCHED[0] : 0) && ks.stop_state == nullptr;
  if (!ok) { ++bad; printf("round trip: mode %d sched %d stop %d\n", k.mode, k.sched, k.stop); }
  expect(!k.stop, ic, fc, false, "without a stop record");   // the tail is a wrong length there
}

void refusals(const Case& k) {
  Ints ic; Floats fc;
  pack(k, &ic, &fc);
  // every pair of lengths: prefixes, and up to two fillers behind the full lists that fit no field
  for (size_t li = 0; li <= ic.size() + 2; ++li)
    for (size_t lf = 0; lf <= fc.size() + 2; ++lf) {
      Ints a(ic.begin(), ic.begin() + std::min(li, ic.size())); a.resize(li, 7);
      Floats b(fc.begin(), fc.begin() + std::min(lf, fc.size())); b.resize(lf, -1.0);
      for (int with_stop = 0; with_stop < 2; ++with_stop) expect(valid(a, b, with_stop), a, b, with_stop, "lengths");
    }
  // the mode flags, from behind: kl_early_stop, lr_schedule, then the mode's own ints
  size_t at = ic.size();
  std::vector<size_t> flags;
  if (k.stop) flags.push_back(--at);
  if (k.sched) flags.push_back(--at);
  if (k.mode == 1) flags.push_back(at - 2);
  for (size_t f : flags)
    for (int64_t v : {0, 2, -1}) { Ints a = ic; a[f] = v; expect(false, a, fc, true, "flag"); }
  if (k.mode == 1) for (int64_t v : {1, 2, -1}) { Ints a = ic; a[at - 1] = v; expect(false, a, fc, true, "shared pair"); }
  if (k.mode >= 2) for (int64_t v : {0, -1}) { Ints a = ic; a[at - 3] = v; expect(false, a, fc, true, "contact_points"); }
  // ints that do not fit 32 bits, at every position
  for (size_t i = 0; i < ic.size(); ++i)
    for (int64_t v : {(int64_t)INT32_MAX + 1, (int64_t)INT32_MIN - 1, (int64_t)1 << 32 | 1, std::numeric_limits<int64_t>::min()}) {
      Ints a = ic; a[i] = v; expect(false, a, fc, true, "wide int");
    }
  // non-positive dimensions and layer counts
  for (size_t i : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)(4 + M), (size_t)(5 + 2 * M), (size_t)(6 + 2 * M), (size_t)(7 + 2 * M)})
    for (int64_t v : {0, -3}) { Ints a = ic; a[i] = v; expect(false, a, fc, true, "dimension"); }
  for (size_t i : {(size_t)3, (size_t)(4 + M)}) { Ints a = ic; a[i] = M + 1; expect(false, a, fc, true, "layer count"); }
  // thresholds and rates
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (k.sched) {
    for (int j = 0; j < 3; ++j)
      for (double v : {nan, 0.0, -0.5}) { Floats b = fc; b[12 + j] = v; expect(false, ic, b, true, "schedule float"); }
    Floats b = fc; b[13] = 2 * b[14]; expect(false, ic, b, true, "lr_min > lr_max");
  }
  if (k.stop) {
    for (double v : {nan, 0.0, -0.5}) { Floats b = fc; b.back() = v; expect(false, ic, b, true, "stop threshold"); }
    if (k.sched) { Floats b = fc; b.back() *= 2; expect(false, ic, b, true, "two thresholds"); }
    Ints a = ic; a[5 + 2 * M] = 1; a[6 + 2 * M] = 3; expect(false, a, fc, true, "fewer samples than mini-epochs");
  }
}
}  // namespace

int main() {
  static_assert(M == 4, "the tables above hold IGI_MAX_LAYERS == 4 widths");
  for (int mode = 0; mode < 4; ++mode)
    for (int sched = 0; sched < 2; ++sched)
      for (int stop = 0; stop < 2; ++stop) {
        const Case k = {mode, sched, stop};
        round_trip(k);
        refusals(k);
      }
  igi_teacher_cfg c;
  char err[64];
  if (igi_teacher_cfg_decode(nullptr, 3, nullptr, 0, &c, nullptr, err, sizeof(err)) != IGI_E_BADARG || !err[0]) { ++bad; printf("null lists\n"); }
  printf("teacher_cfg_check: %lld accepted, %lld refusals, %lld bad\n", accepted, refused, bad);
  return bad ? 1 : 0;
}
