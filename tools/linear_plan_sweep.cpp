// The dense layers' launch plan under the host sanitizers (tools only, not part of librgnn.so; needs no GPU).  Walks the grid of
// tests/linear_dispatch_cases.py with operand "addresses" that are odd, tiny or NULL -- nothing is mapped behind any of them, so a
// plan that read through a pointer would fault -- and prints how many argument sets each kernel family takes.  The sanitizers go on
// the HOST code only (the device code is compiled as always and never runs):
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in linear linear_dma core; do hipcc $F -c radargnn_amd/csrc/$f.hip -o /tmp/lp_$f.o; done
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -c tools/linear_plan_sweep.cpp -o /tmp/lp_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/lp_*.o -o tools/linear_plan_sweep.bin && tools/linear_plan_sweep.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../include/rgnn.h"

static const float* fp(uintptr_t v) { return (const float*)v; }

int main() {
  const int64_t ms[] = {1, 255, 3000, 4096, 192000};
  const int ns[] = {4, 16, 32, 33, 36, 64, 68, 96, 100, 128, 160, 224, 256, 272, 464, 928};
  const int k1s[] = {4, 5, 8, 16, 32, 48, 128, 224, 512, 528, 1024}, k2s[] = {0, 4, 16, 32};
  // operand bases: 16-byte aligned but unmapped, misaligned by 4, odd, and (where the call allows it) NULL
  const uintptr_t bases[] = {0x1000, 0x1004, 0x1001, 0};
  const char* envs[] = {nullptr, "RGNN_LINEAR_FP32", "RGNN_X3_NODMA", "RGNN_LINEAR_NO_F16", "RGNN_DMA_NO_SMALL_M"};
  long families[5] = {0, 0, 0, 0, 0}, fused = 0, total = 0;
  for (const char* env : envs) {
    if (env) setenv(env, "1", 1);
    rgnn_env_reload();
    for (int64_t m : ms) for (int n : ns) for (int k1 : k1s) for (int k2 : k2s)
      for (uintptr_t base : bases) for (int flags = 0; flags < 64; flags++) {
        rgnn_linear_args a = {};
        a.A1 = fp(base); a.lda1 = k1; a.k1 = k1; a.A2 = k2 ? fp(base + 0x100) : nullptr; a.lda2 = k2; a.k2 = k2;
        a.W1 = fp(base ? base + 0x200 : 0x200); a.ldw = k1 + k2; a.w_split = n; a.bias1 = fp(base);
        a.out = (float*)(base ? base + 0x300 : 0x300); a.ldo = n; a.m = m; a.n = n; a.relu_out = 1;
        if (flags & 1) { a.W_planes = fp(base + 0x400); a.w_planes_kp = rgnn_linear_planes_kp(k1 + k2); }
        if (flags & 2) { a.W_planes_f16 = fp(base + 0x500); a.a1_bound = fp(base + 0x600); a.a2_bound = fp(base + 0x700); }
        if (flags & 4) { a.row_index = (const int32_t*)(base + 0x800); a.m_dev = (const int64_t*)(base + 0x900); }
        if (flags & 8) a.col_stats = (float*)(base + 0xa00);
        if (flags & 16) { a.a1_scale_shift = fp(base + 0xb00); if (flags & 4) a.a1_panel_segment = (const int32_t*)(base + 0xc00); }
        if (flags & 32) { a.splitk_ws = (void*)(base + 0xd00); a.splitk_ws_bytes = rgnn_linear_splitk_ws_bytes(); a.relu_from_col = 8; }
        int32_t plan[8];
        rgnn_linear_fwd_plan(&a, plan);
        const int32_t path = rgnn_linear_fwd_path(&a), fuses = rgnn_linear_fwd_fuses_a1_affine(&a);
        if (path != (plan[0] == RGNN_LINEAR_FAMILY_DMA ? plan[1] : 0) || fuses != plan[6] || plan[0] < 0 || plan[0] > 4) {
          printf("the three views disagree: m %lld n %d k1 %d k2 %d base %#lx flags %d\n", (long long)m, n, k1, k2, (unsigned long)base, flags);
          return 1;
        }
        families[plan[0]]++; fused += fuses; total++;
      }
    if (env) unsetenv(env);
  }
  int32_t none[8];
  rgnn_linear_fwd_plan(nullptr, none);
  printf("%ld argument sets: none %ld, tiny %ld, fp32 %ld, x3 %ld, dma %ld; a1 affine fused %ld\n", total, families[0], families[1],
         families[2], families[3], families[4], fused);
  return 0;
}
