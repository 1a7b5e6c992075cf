// What does ONE global_load_dwordx4 gather cost the vector L1 as a function of the 128-byte lines its 64 lanes touch?
// (gfx950; the filter's L1-served table look-ups.)  Every lane reads the 16-byte entry idx[lane] of a 4 KiB table
// (32 lines, L1-resident after the first touch), the same pattern again and again, 16 waves per CU so that the L1 is
// the bound; one launch per pattern.  With `stream`, every gather is followed by a coalesced 1 KiB load (16 bytes per
// lane) that misses L1 and hits L2 -- the code-word stream of the filter kernel.
//   hipcc --offload-arch=gfx950 -O3 scripts/micro/l1_gather.hip -o /tmp/l1_gather && /tmp/l1_gather > l1_gather.txt
// Output: name, distinct lines, cycles per gather wave-instruction and CU (2.4 GHz), the 64 entry numbers.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
#include <set>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int STREAM_UNITS = 1 << 16;   // 16-byte units of the stream buffer (1 MiB: past L1, inside L2)

template <bool STREAM>
__global__ __launch_bounds__(1024) void probe(const int *__restrict__ idx, const uint4 *__restrict__ table,
                                              const uint4 *__restrict__ stream, int iters, uint4 *__restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int gwave = blockIdx.x * 16 + (tid >> 6);
  int a = idx[lane];                              // < 256
  uint32_t acc = 0;
  uint32_t s = (uint32_t)gwave * 37u * 64u;       // this wave's place in the stream, in 16-byte units
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < 16; u++) {
      asm volatile("" : "+v"(a));
      const uint4 x = table[a];
      acc += x.x + x.y + x.z + x.w;
      if (STREAM) {
        const uint4 y = stream[(s + lane) & (STREAM_UNITS - 1)];
        acc += y.x + y.y + y.z + y.w;
        s += 64;
      }
    }
  }
  out[(size_t)blockIdx.x * 1024 + tid] = make_uint4(acc, 0, 0, 0);
}

int main() {
  const int blocks = 256, iters = 200;
  int *d_idx; uint4 *tab, *str, *o;
  CK(hipMalloc(&d_idx, 64 * 4)); CK(hipMalloc(&tab, 4096)); CK(hipMalloc(&str, (size_t)STREAM_UNITS * 16));
  CK(hipMalloc(&o, (size_t)blocks * 1024 * sizeof(uint4)));
  CK(hipMemset(tab, 1, 4096)); CK(hipMemset(str, 1, (size_t)STREAM_UNITS * 16));
  std::vector<std::vector<int>> pats;
  std::vector<const char *> names;
  auto add = [&](const char *nm, std::vector<int> p) { pats.push_back(p); names.push_back(nm); };
  std::mt19937 rng(7);
  std::vector<int> p(64);
  // L distinct lines of the table's 32; the entry inside its line (8 per line) varies from lane to lane
  for (int L : {1, 2, 3, 4, 8, 16, 28, 29, 30, 31, 32}) {
    // equal lines in neighbouring lanes ...
    for (int l = 0; l < 64; l++) p[l] = ((l * L / 64) * (32 / L)) % 32 * 8 + (l * 5 + 3) % 8;
    add("near", p);
    // ... scattered over the wave ...
    for (int l = 0; l < 64; l++) p[l] = ((l % L) * (32 / L)) % 32 * 8 + (l * 5 + 3) % 8;
    add("scat", p);
    // ... and neighbouring with every lane of a line on the SAME 16 bytes
    for (int l = 0; l < 64; l++) p[l] = ((l * L / 64) * (32 / L)) % 32 * 8;
    add("near_same", p);
  }
  // what the kernel does today: 64 random entries of the 256
  for (int r = 0; r < 6; r++) { for (int l = 0; l < 64; l++) p[l] = rng() % 256; add("rand256", p); }
  // a sorted window's second key: three values, in runs
  for (int r = 0; r < 3; r++) { const int c0 = rng() % 254; for (int l = 0; l < 64; l++) p[l] = c0 + (l * 3 / 64); add("runs3", p); }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int stream = 0; stream < 2; stream++)
    for (size_t i = 0; i < pats.size(); i++) {
      for (int l = 0; l < 64; l++) if (pats[i][l] < 0 || pats[i][l] > 255) { printf("bad pattern\n"); return 1; }
      CK(hipMemcpy(d_idx, pats[i].data(), 64 * 4, hipMemcpyHostToDevice));
      float best = 1e9f;
      for (int rep = 0; rep < 3; rep++) {
        CK(hipEventRecord(e0));
        if (stream) hipLaunchKernelGGL(probe<true>, dim3(blocks), dim3(1024), 0, 0, d_idx, tab, str, iters, o);
        else hipLaunchKernelGGL(probe<false>, dim3(blocks), dim3(1024), 0, 0, d_idx, tab, str, iters, o);
        CK(hipGetLastError());
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
      }
      std::set<int> lines;
      for (int l = 0; l < 64; l++) lines.insert(pats[i][l] / 8);
      const double winst = 16.0 * iters * 16;
      printf("%s%s %d %.2f", names[i], stream ? "+stream" : "", (int)lines.size(), best * 1e6 / winst * 2.4);
      for (int l = 0; l < 64; l++) printf(" %d", pats[i][l]);
      printf("\n");
    }
  return 0;
}
