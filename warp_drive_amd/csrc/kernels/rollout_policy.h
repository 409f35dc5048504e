// rollout_policy.h -- the small network that runs INSIDE the rollout and evaluation kernels, written once: two hidden
// layers of H ReLU units, then one softmax head or one tanh actor head, the weights in LDS (every lane reads the same
// address: broadcast), the activations in registers.  Included by cartpole_common.h (the main code object and
// wd_kernels_cp_pool.hsaco), classic_control.hip (wd_kernels_cc.hsaco) and tag_gridworld_n5_common.h
// (wd_kernels_gw5.hsaco, wd_kernels_gw5_pool.hsaco).  Templates only; nothing here reads a unit's macro or constant.
// A change here changes all five objects: compare their disassembly per entry as profiles/r29_rollout_policy_asm_diff.txt did.
//
// PARITY CONTRACT (the host restatements are the independent side of the tolerance-0 tests and share nothing with this
// file: oracle/cartpole_np.py::policy_probabilities, tests/classic_control_policy.py::policy_probabilities,
// tests/classic_control_actor.py::actor_mean_f32, oracle/tag_gridworld_np.py::policy_probabilities):
//   * every unit: acc = bias, then ONE fmaf per input in index order (float32), ReLU as fmaxf(acc, 0);
//   * softmax head: the logits as above, their maximum subtracted, expf, the sum of the terms in action order starting
//     from 0, ONE division e[a] / sum per action.  Slots at or past n_actions hold 0 and add +0 to the sum;
//   * running sums (what the inverse-CDF draw compares the uniform with, random.cu:51-85): cum = p[0], then cum + p[a]
//     in action order, the last value repeated up to the bound;
//   * counting draw: the number of running sums < u, clamped to n_actions - 1; greedy: the FIRST maximum (strict '<');
//   * actor head: z = ba + Wa . h2 (the same fmaf chain), mean = fmaf(scale, tanhf(z), bias);
//   * OU step: normal = sqrtf(-2 logf(u1)) cosf(2 pi u2) of the two uniforms of Philox counter {row, epoch, tag, 1},
//     ou = (1 - damping) ou + stddev normal.
//
// PACKED WEIGHTS (training/policy_kernel.py), all float32, in this order:
//   softmax policy  W0 [H][I], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A]      rp_policy_floats(I, H, A)
//   actor           W0 [H][OP], b0 [H], W1 [H][H], b1 [H], Wa [H], ba [1]        rp_actor_floats(H, O)
// I = floats per row of W0: the observation size, or a padded stride (TagGridWorld: 24 for 21 inputs; OP = O rounded up
// to even for the actor: the pad column is zero and the pad input is 0, so the pad adds +0 exactly).
//
// WHERE THE PIECES STAND.  Here: the first layers, one per input form (rp_first_layer*); the second layer; the logits;
// the probabilities; the actor head; the greedy scan; the float counts.  A unit calls its first layer, then
// rp_policy_logits / rp_actor_mean with the pointer BEHIND b0 and the first activations.  In the units, because behind a
// call their entries compile to another schedule or register numbering (docs/rounds/r29.md lists what was tried): the
// running sums with the softmax terms in front of them (cp_policy_cum, cc_policy_cum: rp_softmax_probs's statements with
// the sum taken next to the division), the float2-row first layer of cc_policy_probs / cc_policy_cum, the counting
// draws, the OU step and the staging copies of the packed weights into LDS.
#pragma once
#include "wd_common.h"

namespace {

constexpr int rp_pad4(int n) { return (n + 3) & ~3; }
constexpr int rp_policy_floats(int I, int H, int A) { return I * H + H + H * H + H + A * H + A; }
constexpr int rp_actor_op(int O) { return (O + 1) & ~1; }
constexpr int rp_actor_floats(int H, int O) { return rp_actor_op(O) * H + H + H * H + H + H + 1; }

// ---- first layers
// the input is one float4 (Cartpole's state), the rows of W0 are one float4 each
template <int H>
__device__ __forceinline__ void rp_first_layer(const float *W0, const float *b0, const float4 &s, float (&h1)[H]) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float4 wr = *(const float4 *)(W0 + 4 * i);
    float acc = b0[i];
    acc = fmaf(wr.x, s.x, acc); acc = fmaf(wr.y, s.y, acc); acc = fmaf(wr.z, s.z, acc); acc = fmaf(wr.w, s.w, acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// an even number O of inputs in registers, the rows of W0 read as float2
template <int H, int O>
__device__ __forceinline__ void rp_first_layer(const float *W0, const float *b0, const float (&o)[O], float (&h1)[H]) {
  static_assert(O % 2 == 0, "the rows of W0 are read as float2");
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
#pragma unroll
    for (int j = 0; j < O; j += 2) {
      const float2 wr = *(const float2 *)(W0 + O * i + j);
      acc = fmaf(wr.x, o[j], acc); acc = fmaf(wr.y, o[j + 1], acc);
    }
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// any O: the input padded with 0 to OP = rp_actor_op(O) floats, rows of OP floats
template <int H, int O>
__device__ __forceinline__ void rp_first_layer_padded(const float *W0, const float *b0, const float (&o)[O],
                                                      float (&h1)[H]) {
  constexpr int OP = rp_actor_op(O);
  float op[OP];
#pragma unroll
  for (int j = 0; j < OP; ++j) op[j] = (j < O) ? o[j < O ? j : 0] : 0.0f;
  rp_first_layer<H, OP>(W0, b0, op, h1);
}

// F inputs read from x (LDS), rows of W0 at STRIDE floats: whole float4s, then the tail columns one by one
template <int H, int F, int STRIDE>
__device__ __forceinline__ void rp_first_layer_strided(const float *W0, const float *b0, const float *x,
                                                       float (&h1)[H]) {
  static_assert(STRIDE % 4 == 0 && STRIDE >= F, "every row of W0 starts on a 16-byte boundary");
  float in[F];
#pragma unroll
  for (int j = 0; j < F; ++j) in[j] = x[j];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
#pragma unroll
    for (int j = 0; j < (F & ~3); j += 4) {
      const float4 wr = *(const float4 *)(W0 + i * STRIDE + j);
      acc = fmaf(wr.x, in[j], acc); acc = fmaf(wr.y, in[j + 1], acc);
      acc = fmaf(wr.z, in[j + 2], acc); acc = fmaf(wr.w, in[j + 3], acc);
    }
#pragma unroll
    for (int j = (F & ~3); j < F; ++j) acc = fmaf(W0[i * STRIDE + j], in[j], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// ---- second hidden layer
template <int H>
__device__ __forceinline__ void rp_second_layer(const float *W1, const float *b1, const float (&h1)[H], float (&h2)[H]) {
  static_assert(H % 4 == 0, "the rows of W1 and of the heads are read as float4");
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b1[i];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(W1 + i * H + j);
      acc = fmaf(wr.x, h1[j], acc); acc = fmaf(wr.y, h1[j + 1], acc);
      acc = fmaf(wr.z, h1[j + 2], acc); acc = fmaf(wr.w, h1[j + 3], acc);
    }
    h2[i] = fmaxf(acc, 0.0f);
  }
}

// ---- softmax head over the compile-time bound MAXA, n_actions <= MAXA of them real ((uniform); a caller whose action
// count is a constant passes it and the guards fold away).  The logits (-inf past n_actions); returns their maximum
template <int H, int MAXA>
__device__ __forceinline__ float rp_logits(const float *Wp, const float *bp, const float (&h2)[H], int n_actions,
                                           float (&logit)[MAXA]) {
  float m = -__builtin_inff();
#pragma unroll
  for (int a = 0; a < MAXA; ++a) {
    logit[a] = -__builtin_inff();
    if (a < n_actions) {
      float acc = bp[a];
#pragma unroll
      for (int j = 0; j < H; j += 4) {
        const float4 wr = *(const float4 *)(Wp + a * H + j);
        acc = fmaf(wr.x, h2[j], acc); acc = fmaf(wr.y, h2[j + 1], acc);
        acc = fmaf(wr.z, h2[j + 2], acc); acc = fmaf(wr.w, h2[j + 3], acc);
      }
      logit[a] = acc;
      m = fmaxf(m, acc);
    }
  }
  return m;
}

// the probabilities of the logits: e[a] = expf(logit[a] - max) (0 past n_actions), their sum in action order,
// prob[a] = e[a] / sum
template <int MAXA>
__device__ __forceinline__ void rp_softmax_probs(const float (&logit)[MAXA], float m, int n_actions, float (&prob)[MAXA]) {
  float e[MAXA], sum = 0.0f;
#pragma unroll
  for (int a = 0; a < MAXA; ++a) {
    e[a] = (a < n_actions) ? expf(logit[a] - m) : 0.0f;
    sum += e[a];
  }
#pragma unroll
  for (int a = 0; a < MAXA; ++a) prob[a] = e[a] / sum;
}

// second layer + logits: w1 = the packed weights behind b0, h1 = the first layer's activations; returns the maximum
template <int H, int MAXA>
__device__ __forceinline__ float rp_policy_logits(const float *w1, const float (&h1)[H], int n_actions,
                                                  float (&logit)[MAXA]) {
  const float *W1 = w1, *b1 = W1 + H * H, *Wp = b1 + H, *bp = Wp + n_actions * H;
  float h2[H];
  rp_second_layer<H>(W1, b1, h1, h2);
  return rp_logits<H>(Wp, bp, h2, n_actions, logit);
}

// second layer + actor head
template <int H>
__device__ __forceinline__ float rp_actor_mean(const float *w1, const float (&h1)[H], float action_scale,
                                               float action_bias) {
  const float *W1 = w1, *b1 = W1 + H * H, *Wa = b1 + H, *ba = Wa + H;
  float h2[H];
  rp_second_layer<H>(W1, b1, h1, h2);
  float z = ba[0];
#pragma unroll
  for (int j = 0; j < H; j += 4) {
    const float4 wr = *(const float4 *)(Wa + j);
    z = fmaf(wr.x, h2[j], z); z = fmaf(wr.y, h2[j + 1], z);
    z = fmaf(wr.z, h2[j + 2], z); z = fmaf(wr.w, h2[j + 3], z);
  }
  return fmaf(action_scale, tanhf(z), action_bias);
}

// the greedy action: the first maximum of the first n_actions probabilities (the standalone sampler's strict-'<' scan)
template <int MAXA>
__device__ __forceinline__ int rp_first_maximum(const float (&prob)[MAXA], int n_actions) {
  int a = 0;
  float best = prob[0];
#pragma unroll
  for (int i = 1; i < MAXA; ++i) {
    const bool better = i < n_actions && best < prob[i];
    best = better ? prob[i] : best;
    a = better ? i : a;
  }
  return a;
}

}  // namespace
