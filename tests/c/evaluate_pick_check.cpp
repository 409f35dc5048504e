// evaluate_pick_check: a HOST program that prints what the action section of include/wd_env_evaluate.h computes -- the
// probabilities of a row of logits, the running sums built from them (next to wd_env_rollout.h's, which they must equal
// bit for bit) and the greedy pick -- so that tests/test_custom_env_evaluate_build.py can hold them against numpy.  Built
// with the host compiler alone: the header reads no HIP header when __HIPCC__ is not defined, and nothing here calls the
// HIP runtime.
//
// Standard input, every number unsigned decimal (floats as their bit patterns): R, then R rows of
//   kind A v[0 .. 8)
// kind 0: v are LOGITS (slots at and past A are ignored: the header's own -inf stands there, as wd_rollout_logits leaves
//         it).  Output: "L p[0 .. 8) cum[0 .. 8) rollout_cum[0 .. 8) pick"
// kind 1: v are PROBABILITIES handed straight to the scan, slots at and past A included.  Output: "S pick"
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wd_env_evaluate.h"

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

int main() {
  int R;
  if (scanf("%d", &R) != 1 || R < 0) return 2;
  for (int r = 0; r < R; ++r) {
    int kind, A;
    if (scanf("%d %d", &kind, &A) != 2) return 2;
    if (kind < 0 || kind > 1 || A < 1 || A > WD_ROLLOUT_MAX_ACTIONS) return 3;
    float v[WD_ROLLOUT_MAX_ACTIONS];
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
      unsigned b;
      if (scanf("%u", &b) != 1) return 2;
      v[a] = float_of(b);
    }
    if (kind == 1) {
      printf("S %d\n", wd_evaluate_first_maximum(v, A));
      continue;
    }
    float logit[WD_ROLLOUT_MAX_ACTIONS], m = -INFINITY;  // as wd_rollout_logits leaves them
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
      logit[a] = -INFINITY;
      if (a < A) {
        logit[a] = v[a];
        m = fmaxf(m, logit[a]);
      }
    }
    float prob[WD_ROLLOUT_MAX_ACTIONS], cum[WD_ROLLOUT_MAX_ACTIONS], rollout_cum[WD_ROLLOUT_MAX_ACTIONS];
    wd_evaluate_probabilities(logit, m, A, prob);
    wd_evaluate_running_sums(prob, A, cum);
    wd_rollout_running_sums(logit, m, A, rollout_cum);
    printf("L");
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) printf(" %u", bits_of(prob[a]));
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) printf(" %u", bits_of(cum[a]));
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) printf(" %u", bits_of(rollout_cum[a]));
    printf(" %d\n", wd_evaluate_first_maximum(prob, A));
  }
  return 0;
}
