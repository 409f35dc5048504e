// tick_draw_check: a HOST program that prints what the fused tick of include/wd_env_tick.h draws -- the Philox block, the
// uniforms and the categorical pick -- so that tests/test_custom_env_tick_build.py can hold them against the numpy model
// bit for bit.  Built with the host compiler alone: the header reads no HIP header when __HIPCC__ is not defined, and
// nothing here calls the HIP runtime.
//
// Commands on standard input, one per line, every number unsigned decimal (floats as their bit patterns):
//   D k0 k1 row epoch tag                      -> "D w0 w1 w2 w3 u0 u1 u2 u3": the block's words and the uniforms' bits
//   P head k0 k1 row epoch tag n p0 .. p(n-1)  -> "P a": the pick of head `head` on that probability row
//   L                                          -> "L size data ref row_elems": the reset entry's layout
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "wd_env_tick.h"

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
  char cmd[8];
  while (scanf("%7s", cmd) == 1) {
    if (cmd[0] == 'L') {
      printf("L %zu %zu %zu %zu\n", sizeof(wd_tick_reset_entry), offsetof(wd_tick_reset_entry, data),
             offsetof(wd_tick_reset_entry, ref), offsetof(wd_tick_reset_entry, row_elems));
    } else if (cmd[0] == 'D') {
      unsigned k0, k1, row, epoch, tag;
      if (scanf("%u %u %u %u %u", &k0, &k1, &row, &epoch, &tag) != 5) return 2;
      const wd_tick_u4 b = wd_tick_block(row, epoch, tag, k0, k1);
      printf("D %u %u %u %u", b.x, b.y, b.z, b.w);
      for (int h = 0; h < WD_TICK_MAX_HEADS; ++h) printf(" %u", bits_of(wd_tick_uniform(wd_tick_word(b, h))));
      printf("\n");
    } else if (cmd[0] == 'P') {
      unsigned head, k0, k1, row, epoch, tag, n;
      if (scanf("%u %u %u %u %u %u %u", &head, &k0, &k1, &row, &epoch, &tag, &n) != 7) return 2;
      if (head >= WD_TICK_MAX_HEADS || n < 1 || n > 4096) return 3;
      std::vector<float> p(n);
      for (unsigned i = 0; i < n; ++i) {
        unsigned b;
        if (scanf("%u", &b) != 1) return 2;
        p[i] = float_of(b);
      }
      const wd_tick_u4 b = wd_tick_block(row, epoch, tag, k0, k1);
      printf("P %d\n", wd_tick_pick(p.data(), (int)n, wd_tick_uniform(wd_tick_word(b, (int)head))));
    } else {
      return 4;
    }
  }
  return 0;
}
