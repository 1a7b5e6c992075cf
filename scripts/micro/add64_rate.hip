// What do the candidate instructions of the prefix block's arithmetic cost the vector ALU next to a plain v_add_u32?
// (gfx950; in the style of mqsad_rate.hip.)  The prefix test of the filter's main stage (filter.hip) adds 16-byte
// table entries dword by dword, widens byte sums to 16 bits and tests sixteen 16-bit sums against QMAX; candidates:
//   * v_lshl_add_u64 with shift 0 as ONE add for two dwords of a byte-sum addition (no carry can cross: bytes <= 255);
//   * v_mad_i32_i24 (x, -256, w) for  w - (x << 8)  in one instruction instead of a shift and a subtraction;
//   * v_pk_min_u16 for a minimum tree over the accumulators instead of one saturating subtraction each.
// 16 waves per CU, one launch per variant, nothing but the chain in the loop:
//   add        : v_add_u32, dependent                                   (the yardstick)
//   add2       : two independent v_add_u32 (what one v_lshl_add_u64 would replace)
//   add64      : v_lshl_add_u64 d, a, 0, d
//   shl_sub    : v_lshlrev_b32 + v_sub_u32 (what one v_mad_i32_i24 would replace)
//   mad_i24    : v_mad_i32_i24 d, x, s(-256), d
//   pk_min     : v_pk_min_u16, dependent
//   pk_sub_sat : v_pk_sub_u16 clamp, dependent
//   hipcc --offload-arch=gfx950 -O3 scripts/micro/add64_rate.hip -o /tmp/add64_rate && /tmp/add64_rate > add64_rate.txt
// Output: name, cycles per chain step and SIMD at 2.4 GHz (4 waves per SIMD), instructions per step, and a check of
// the arithmetic of add64 and mad_i24 against the host.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int UNROLL = 32;
constexpr int NVAR = 7;

template <int VARIANT>
__global__ __launch_bounds__(1024) void probe(const uint32_t *__restrict__ in, int iters, int k, uint4 *__restrict__ out) {
  const int tid = threadIdx.x;
  uint32_t x = in[tid & 63], y = in[(tid + 1) & 63];
  uint32_t a = 0, b = 0;
  uint64_t w = 0;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      asm volatile("" : "+v"(x), "+v"(y), "+v"(a), "+v"(b), "+v"(w));   // (opaque: nothing folded across steps)
      if (VARIANT == 0) {
        a += x;
      } else if (VARIANT == 1) {
        a += x;
        b += y;
      } else if (VARIANT == 2) {
        asm("v_lshl_add_u64 %0, %1, 0, %0" : "+v"(w) : "v"(((uint64_t)y << 32) | x));
      } else if (VARIANT == 3) {
        a = a - (x << 8);
      } else if (VARIANT == 4) {
        asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(a) : "v"(x), "s"(k));
      } else if (VARIANT == 5) {
        asm("v_pk_min_u16 %0, %0, %1" : "+v"(a) : "v"(x));
      } else {
        asm("v_pk_sub_u16 %0, %0, %1 clamp" : "+v"(a) : "v"(x));
      }
    }
  }
  out[(size_t)blockIdx.x * 1024 + tid] = make_uint4((uint32_t)w, (uint32_t)(w >> 32), a, b);
}

int main() {
  const int blocks = 256, iters = 2000;
  uint32_t h_in[64];
  for (int l = 0; l < 64; l++) h_in[l] = 0x01020304u * (uint32_t)(l % 60) + 0x00010203u;   // bytes <= 240
  uint32_t *d_in; uint4 *o;
  CK(hipMalloc(&d_in, sizeof(h_in))); CK(hipMalloc(&o, (size_t)blocks * 1024 * sizeof(uint4)));
  CK(hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char *names[NVAR] = {"add", "add2", "add64", "shl_sub", "mad_i24", "pk_min", "pk_sub_sat"};
  const int per_step[NVAR] = {1, 2, 1, 2, 1, 1, 1};
  for (int v = 0; v < NVAR; v++) {
    float best = 1e9f;
    for (int rep = 0; rep < 3; rep++) {
      CK(hipEventRecord(e0));
      const dim3 g(blocks), t(1024);
      if (v == 0) hipLaunchKernelGGL(probe<0>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 1) hipLaunchKernelGGL(probe<1>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 2) hipLaunchKernelGGL(probe<2>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 3) hipLaunchKernelGGL(probe<3>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 4) hipLaunchKernelGGL(probe<4>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 5) hipLaunchKernelGGL(probe<5>, g, t, 0, 0, d_in, iters, -256, o);
      if (v == 6) hipLaunchKernelGGL(probe<6>, g, t, 0, 0, d_in, iters, -256, o);
      CK(hipGetLastError());
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep > 0 && ms < best) best = ms;
    }
    // 256 workgroups of 16 waves on 256 CUs: 4 waves per SIMD
    const double steps_per_simd = 4.0 * (double)iters * UNROLL;
    printf("%s %.2f cycles per chain step and SIMD, %d instructions per step\n", names[v],
           best * 1e-3 * 2.4e9 / steps_per_simd, per_step[v]);
    if (v == 2 || v == 4) {
      uint4 h; CK(hipMemcpy(&h, o + 5, sizeof(h), hipMemcpyDeviceToHost));
      const uint64_t steps = (uint64_t)iters * UNROLL;
      if (v == 2) {   // one 64-bit sum of (in[6] : in[5]), steps times
        const uint64_t got = ((uint64_t)h.y << 32) | h.x, want = steps * (((uint64_t)h_in[6] << 32) | h_in[5]);
        printf("  arithmetic %s (got %016llx, want %016llx)\n", got == want ? "ok" : "WRONG", (unsigned long long)got,
               (unsigned long long)want);
      } else {        // a - (x << 8) per step, mod 2^32, from x's low 24 bits alone
        const uint32_t want = (uint32_t)(0u - (uint32_t)steps * (h_in[5] << 8));
        printf("  arithmetic %s (got %08x, want %08x)\n", h.z == want ? "ok" : "WRONG", h.z, want);
      }
    }
  }
  return 0;
}
