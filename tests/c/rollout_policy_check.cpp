// rollout_policy_check: a HOST program that prints what the in-kernel policy of include/wd_env_rollout.h computes -- the
// logits, the running sums of their softmax and the pick -- so that tests/test_custom_env_rollout_build.py can hold them
// against the numpy model.  Built with the host compiler alone: the header reads no HIP header when __HIPCC__ is not
// defined, and nothing here calls the HIP runtime.
//
// Standard input, every number unsigned decimal (floats as their bit patterns):
//   H F A R, then wd_rollout_policy_floats(F, H, A) packed weights, then R rows of F observation floats and one uniform
// Output, one line per row: "R logit[0 .. A) cum[0 .. A) pick".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "wd_env_rollout.h"

static uint32_t bits_of(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

static float float_of(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}

static bool read_float(float *out) {
  unsigned b;
  if (scanf("%u", &b) != 1) return false;
  *out = float_of(b);
  return true;
}

template <int H, int F>
static int rows(const float *w, int A, int R) {
  for (int r = 0; r < R; ++r) {
    float obs[F], u;
    for (int j = 0; j < F; ++j)
      if (!read_float(&obs[j])) return 2;
    if (!read_float(&u)) return 2;
    float logit[WD_ROLLOUT_MAX_ACTIONS], cum[WD_ROLLOUT_MAX_ACTIONS];
    const float m = wd_rollout_logits<H, F>(w, obs, A, logit);
    wd_rollout_running_sums(logit, m, A, cum);
    printf("R");
    for (int a = 0; a < A; ++a) printf(" %u", bits_of(logit[a]));
    for (int a = 0; a < A; ++a) printf(" %u", bits_of(cum[a]));
    printf(" %d\n", wd_rollout_pick(cum, A, u));
  }
  return 0;
}

int main() {
  int H, F, A, R;
  if (scanf("%d %d %d %d", &H, &F, &A, &R) != 4) return 2;
  if (A < 1 || A > WD_ROLLOUT_MAX_ACTIONS || R < 0 || H < 4 || H > 64 || F < 1 || F > 7) return 3;
  std::vector<float> w(wd_rollout_policy_floats(F, H, A));
  for (float &v : w)
    if (!read_float(&v)) return 2;
  // the worked example (F = 5), tests/custom_envs/policy_probe.hip (F = 2) ...
  if (H == 32 && F == 5) return rows<32, 5>(w.data(), A, R);
  if (H == 64 && F == 5) return rows<64, 5>(w.data(), A, R);
  if (H == 32 && F == 2) return rows<32, 2>(w.data(), A, R);
  if (H == 64 && F == 2) return rows<64, 2>(w.data(), A, R);
  // ... and the (F, H) of tests/custom_envs/contract_probe.hip
  if (H == 4 && F == 1) return rows<4, 1>(w.data(), A, R);
  if (H == 32 && F == 1) return rows<32, 1>(w.data(), A, R);
  if (H == 32 && F == 4) return rows<32, 4>(w.data(), A, R);
  if (H == 32 && F == 7) return rows<32, 7>(w.data(), A, R);
  if (H == 64 && F == 7) return rows<64, 7>(w.data(), A, R);
  return 3;
}
