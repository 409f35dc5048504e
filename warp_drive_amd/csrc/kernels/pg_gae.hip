// pg_gae.hip -- GAE(lambda) advantages of the A2C / PPO update on the kernels path, in the returns launch's position
// (training/pg_update_kernels.py::_PgUpdateLaunches.gae_returns, the policy key `gae_lambda`): what
// training/losses.py::gae_returns computes on [T][C] arrays (C = E * n columns; column c belongs to replica c / n),
//
//     A[T-1] = d (r[T-1] - V[T-1])                               (R[T-1] = d r + (1 - d) V[T-1], the project's end-of-batch rule)
//     A[t]   = delta_t + gamma lambda (1 - d_t) A[t+1],          delta_t = r[t] + gamma (1 - d_t) V[t+1] - V[t],
//     returns = A + V,   advantages = returns - V,               d = done > 0, the replica's flag
//
// (lambda = 1: returns is HipDiscountedReturns' R).  Nothing here knows a network: one entry serves every user of the
// update launches.
//
// THE SCAN.  A step is the affine map f_t(x) = b_t + a_t x with a_t = gamma lambda (1 - d_t), b_t = delta_t (the last row:
// a = 0, b = d (r - V)), and A[t] = (f_t o f_{t+1} o ... o f_{T-1})(anything).  Maps compose -- (a, b) o (P, Q) =
// (a P, b + a Q) -- so time is cut into segments that are walked at once.
//
// WORK SPLIT.  A block owns a tile of 64 consecutive columns and has S wavefronts (blockDim.x = 64 S, S = 1 .. 16; the host
// picks 1, 2, 4, 8 or 16: `gae_wavefronts`).  Lanes are columns: a wavefront's access to a row is one 256-byte line (a
// replica's done flag is one address for its n lanes).  Wavefront w owns the ticks w L .. min(T, (w + 1) L) - 1,
// L = ceil(T / S); with S > T the last wavefronts own nothing.
//   1. SEGMENT PASS: the wavefront walks its segment backwards once, forms (a_t, b_t) per row and composes the segment's
//      map (P, Q) in registers.  V[t+1] is the row before's V[t]: three loads a row.  A segment of up to 32 rows keeps its
//      pairs in registers (64 VGPRs); rows come in batches of 8 whose loads are issued together, the row index clamped into
//      the segment so that a batch has no branch inside.
//   2. CARRY PASS (S > 1): the maps go to LDS as [S][64] float2; ONE block barrier; wavefront w applies the maps of the
//      segments after its own to 0, last segment first, and so holds A at its segment's upper edge.  The last segment
//      holds row T - 1, whose map is a constant: its own carry (0) is never used.
//   3. WRITE PASS: the wavefront re-walks its segment from the carry, x = b_t + a_t x, and stores x + V[t] and
//      (x + V[t]) - V[t].  Kept pairs: one load a row (V[t]); else the three loads again.
// The dependent chain of a lane is 2 L + S steps instead of T.  S = 1: no LDS, no barrier, a segment too long to keep is walked
// once (pass 3 alone), and the operations are the framework's loop's in its order.  No atomics, no contraction (the build's flags), and for a given (T, S) a fixed
// order: a launch writes the same bytes every time.  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#define PGAE_TILE 64
#define PGAE_MAX_WAVES 16
#define PGAE_KEEP 32    // rows of a segment whose (a, b) stay in registers
#define PGAE_BATCH 8    // rows whose loads are issued together

// the map of one row; `last`: row T - 1 (then vnext is not a value of the batch and is not used)
__device__ __forceinline__ void pgae_map(float r, float v, float vnext, int done, bool last, float gamma, float gl, float &a,
                                         float &b) {
  const float d = done > 0 ? 1.0f : 0.0f, nd = 1.0f - d;
  a = last ? 0.0f : nd * gl;
  b = last ? d * (r - v) : (r + (nd * gamma) * vnext) - v;
}

extern "C" {

// grid = ceil(E n / 64) blocks of 64 S threads, 512 S bytes of dynamic LDS when S > 1 (none for S = 1); a launch with
// another block shape, or T, E, n < 1, touches nothing
__global__ void __launch_bounds__(PGAE_TILE *PGAE_MAX_WAVES) HipPgGaeReturns(
    const float *__restrict__ rewards, const int *__restrict__ done, const float *__restrict__ values, float gamma,
    float lambda, int T, int E, int n, float *__restrict__ returns, float *__restrict__ advantages) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pgae_smem[];
  float2 *const maps = (float2 *)pgae_smem;   // [S][64]: (P, Q) of every segment
  const int S = (int)(blockDim.x >> 6);
  const long C = (long)E * (long)n, first = (long)blockIdx.x * PGAE_TILE;
  if ((blockDim.x & 63) != 0 || S < 1 || S > PGAE_MAX_WAVES || T < 1 || E < 1 || n < 1 || first >= C) return;
  const int lane = (int)(threadIdx.x & 63), w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool live = first + lane < C;
  const long c = live ? first + lane : C - 1;   // (a lane past the last column reads the last one and stores nothing)
  const float *const r_col = rewards + c, *const v_col = values + c;
  const int *const d_col = done + c / n;
  const int L = (T + S - 1) / S, segments = (T + L - 1) / L;
  const int lo = w * L, hi = min(T, lo + L), len = hi - lo;   // (len <= 0: nothing to walk, but the barrier is kept)
  const float gl = gamma * lambda;
  const bool kept = len <= PGAE_KEEP;

  // ---- 1. the segment's map
  float P = 1.0f, Q = 0.0f, a[PGAE_KEEP], b[PGAE_KEEP];
  if (len > 0) {
    float vnext = v_col[(long)min(hi, T - 1) * C];
    if (kept) {
#pragma unroll
      for (int k = 0; k < PGAE_KEEP; k += PGAE_BATCH) {
        if (k < len) {
          float r[PGAE_BATCH], v[PGAE_BATCH];
          int d[PGAE_BATCH];
#pragma unroll
          for (int j = 0; j < PGAE_BATCH; ++j) {
            const long t = max(lo, hi - 1 - (k + j));
            r[j] = r_col[t * C], v[j] = v_col[t * C], d[j] = d_col[t * (long)E];
          }
#pragma unroll
          for (int j = 0; j < PGAE_BATCH; ++j) {
            const int i = k + j;
            pgae_map(r[j], v[j], vnext, d[j], hi - 1 - i == T - 1, gamma, gl, a[i], b[i]);
            if (i < len) Q = b[i] + a[i] * Q, P = a[i] * P, vnext = v[j];
          }
        }
      }
    } else if (S > 1) {   // (S = 1: nobody asks for the map of the one segment, and its rows are read in pass 3)
#pragma unroll 4
      for (int t = hi - 1; t >= lo; --t) {
        const float v = v_col[(long)t * C];
        float at, bt;
        pgae_map(r_col[(long)t * C], v, vnext, d_col[(long)t * E], t == T - 1, gamma, gl, at, bt);
        Q = bt + at * Q, P = at * P, vnext = v;
      }
    }
  }

  // ---- 2. A at the segment's upper edge
  float x = 0.0f;
  if (S > 1) {
    maps[w * PGAE_TILE + lane] = make_float2(P, Q);
    __syncthreads();
    for (int s = segments - 1; s > w; --s) {
      const float2 m = maps[s * PGAE_TILE + lane];
      x = m.y + m.x * x;
    }
  }
  if (len <= 0) return;

  // ---- 3. the segment's rows from the carry
  if (kept) {
#pragma unroll
    for (int k = 0; k < PGAE_KEEP; k += PGAE_BATCH) {
      if (k < len) {
        float v[PGAE_BATCH];
#pragma unroll
        for (int j = 0; j < PGAE_BATCH; ++j) v[j] = v_col[(long)max(lo, hi - 1 - (k + j)) * C];
#pragma unroll
        for (int j = 0; j < PGAE_BATCH; ++j) {
          const int i = k + j;
          if (i < len) {
            x = b[i] + a[i] * x;
            const float ret = x + v[j];
            if (live) {
              const long at = (long)(hi - 1 - i) * C + c;
              returns[at] = ret;
              advantages[at] = ret - v[j];
            }
          }
        }
      }
    }
  } else {
    float vnext = v_col[(long)min(hi, T - 1) * C];
#pragma unroll 4
    for (int t = hi - 1; t >= lo; --t) {
      const float v = v_col[(long)t * C];
      float at, bt;
      pgae_map(r_col[(long)t * C], v, vnext, d_col[(long)t * E], t == T - 1, gamma, gl, at, bt);
      x = bt + at * x, vnext = v;
      const float ret = x + v;
      if (live) {
        returns[(long)t * C + c] = ret;
        advantages[(long)t * C + c] = ret - v;
      }
    }
  }
}

}  // extern "C"
