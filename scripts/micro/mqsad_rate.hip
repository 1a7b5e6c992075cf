// What does ONE v_mqsad_pk_u16_u8 cost the vector ALU next to the instructions it would replace in the filter's
// byte-sum widening?  (gfx950.)  With the reference operand 0x000000FF only byte 0 of the reference is unmasked, so
//   D.u16[i] = acc.u16[i] + 255 - S0.byte[i],  i = 0..3
// widens and accumulates the four byte sums of a dword in one instruction, where the filter kernel spends a v_perm_b32
// and two adds.  16 waves per CU, one launch per variant, nothing but the chain in the loop:
//   add        : v_add_u32, dependent                          (the yardstick)
//   mqsad_dep  : v_mqsad_pk_u16_u8, accumulator chained
//   mqsad_ind  : four independent accumulators, round robin
//   perm_add2  : v_perm_b32 + 2 x v_add_u32 (what one dword costs today)
//   hipcc --offload-arch=gfx950 -O3 scripts/micro/mqsad_rate.hip -o /tmp/mqsad_rate && /tmp/mqsad_rate > mqsad_rate.txt
// Output: name, cycles per wave-instruction and SIMD at 2.4 GHz (4 waves per SIMD), instructions per chain step,
// and a check of the arithmetic against the host.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int UNROLL = 32;

template <int VARIANT>
__global__ __launch_bounds__(1024) void probe(const uint32_t *__restrict__ in, int iters, uint4 *__restrict__ out) {
  const int tid = threadIdx.x;
  uint32_t x = in[tid & 63];
  uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  uint32_t e = 0, o = 0;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      asm volatile("" : "+v"(x), "+v"(e), "+v"(o));   // (opaque: no add3 across steps, no hoisted v_perm_b32)
      if (VARIANT == 0) {
        e += x;
      } else if (VARIANT == 1) {
        a0 = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)x, 0xFFu, a0);
      } else if (VARIANT == 2) {
        if ((u & 3) == 0) a0 = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)x, 0xFFu, a0);
        if ((u & 3) == 1) a1 = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)x, 0xFFu, a1);
        if ((u & 3) == 2) a2 = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)x, 0xFFu, a2);
        if ((u & 3) == 3) a3 = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)x, 0xFFu, a3);
      } else {
        e += x;
        o += __builtin_amdgcn_perm(0u, x, 0x0C030C01u);
      }
    }
  }
  const uint64_t a = a0 + a1 + a2 + a3;
  out[(size_t)blockIdx.x * 1024 + tid] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), e, o);
}

int main() {
  const int blocks = 256, iters = 2000;
  uint32_t h_in[64];
  for (int l = 0; l < 64; l++) h_in[l] = 0x01020304u * (uint32_t)(l % 60) + 0x00010203u;   // bytes <= 240
  uint32_t *d_in; uint4 *o;
  CK(hipMalloc(&d_in, sizeof(h_in))); CK(hipMalloc(&o, (size_t)blocks * 1024 * sizeof(uint4)));
  CK(hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char *names[4] = {"add", "mqsad_dep", "mqsad_ind", "perm_add2"};
  const int per_step[4] = {1, 1, 1, 3};
  for (int v = 0; v < 4; v++) {
    float best = 1e9f;
    for (int rep = 0; rep < 3; rep++) {
      CK(hipEventRecord(e0));
      if (v == 0) hipLaunchKernelGGL(probe<0>, dim3(blocks), dim3(1024), 0, 0, d_in, iters, o);
      if (v == 1) hipLaunchKernelGGL(probe<1>, dim3(blocks), dim3(1024), 0, 0, d_in, iters, o);
      if (v == 2) hipLaunchKernelGGL(probe<2>, dim3(blocks), dim3(1024), 0, 0, d_in, iters, o);
      if (v == 3) hipLaunchKernelGGL(probe<3>, dim3(blocks), dim3(1024), 0, 0, d_in, iters, o);
      CK(hipGetLastError());
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep > 0 && ms < best) best = ms;
    }
    // 256 workgroups of 16 waves on 256 CUs: 4 waves per SIMD
    const double steps_per_simd = 4.0 * (double)iters * UNROLL;
    printf("%s %.2f cycles per chain step and SIMD, %d instructions per step\n", names[v],
           best * 1e-3 * 2.4e9 / steps_per_simd, per_step[v]);
    if (v == 1) {   // the arithmetic: the 16-bit lanes hold (steps * (255 - byte)) mod 2^16
      uint4 h; CK(hipMemcpy(&h, o + 5, sizeof(h), hipMemcpyDeviceToHost));
      const uint64_t got = ((uint64_t)h.y << 32) | h.x;
      uint64_t want = 0;
      for (int i = 0; i < 4; i++) {
        const uint32_t byte = (h_in[5] >> (8 * i)) & 255u;
        want |= (uint64_t)(((uint32_t)iters * UNROLL * (255u - byte)) & 0xFFFFu) << (16 * i);
      }
      printf("  arithmetic %s (got %016llx, want %016llx)\n", got == want ? "ok" : "WRONG", (unsigned long long)got,
             (unsigned long long)want);
    }
  }
  return 0;
}
