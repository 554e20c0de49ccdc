// Measured integer-VALU peak on gfx950: throughput of the instructions the all-pairs
// kernel issues (v_bitop3_b32, v_bcnt_u32_b32, v_xor_b32) in long independent
// chains, all CUs busy, plus the in-kernel clock (s_memtime / s_memrealtime).
//   hipcc --offload-arch=gfx950 -O3 tools/valu_peak.hip -o tools/valu_peak && tools/valu_peak
//   tools/valu_peak --mfma-hold: only the VALU-beside-int8-MFMA cases (hold_k below)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHK(x)                                                                   \
  do {                                                                           \
    hipError_t e = (x);                                                          \
    if (e != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                     \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

constexpr int ITERS = 4096;
constexpr int CH = 12;  // independent chains per lane

template <int OP>
__global__ __launch_bounds__(256) void k(uint32_t* out, uint64_t* clk, uint32_t seed) {
  uint32_t x[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) x[c] = seed * (threadIdx.x + 1) + c * 0x9E3779B9u;
  const uint32_t y = seed ^ threadIdx.x, z = seed + blockIdx.x;
  double dacc[CH];  // OPs 18-20: fp64 accumulate of a square
#pragma unroll
  for (int c = 0; c < CH; ++c) dacc[c] = (double)x[c];
  const double dz = (double)(int)z;
  uint64_t t0 = __builtin_amdgcn_s_memtime();
  uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < ITERS; ++i) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if constexpr (OP == 0) x[c] = __builtin_amdgcn_bitop3_b32(x[c], y, z, 0x96);
      if constexpr (OP == 1) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 2) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 4) asm volatile("v_xor_b32_e64 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 5) asm volatile("v_add3_u32 %0, %1, %2, %0" : "+v"(x[c]) : "v"(y), "v"(z));
      if constexpr (OP == 6) asm volatile("v_or3_b32 %0, %1, %2, %0" : "+v"(x[c]) : "v"(y), "v"(z));
      if constexpr (OP == 7) {  // alternate 8-byte and 4-byte encodings
        asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
        asm volatile("v_xor_b32 %0, %1, %0" : "+v"(x[c]) : "v"(z));
      }
      if constexpr (OP == 8) asm volatile("v_add_u32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 9) asm volatile("v_and_b32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 10) {  // 64-bit accumulate of a square: v_mad_i64_i32
        uint64_t a64 = ((uint64_t)x[c] << 32) | y;
        asm volatile("v_mad_i64_i32 %0, vcc, %1, %1, %0" : "+v"(a64) : "v"(z) : "vcc");
        x[c] = (uint32_t)a64 ^ (uint32_t)(a64 >> 32);
      }
      if constexpr (OP == 11) asm volatile("v_mul_i32_i24 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 12) asm volatile("v_mul_hi_i32_i24 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 13) asm volatile("v_lshl_add_u32 %0, %1, 8, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 14) asm volatile("v_perm_b32 %0, %1, %0, %2" : "+v"(x[c]) : "v"(y), "v"(z));
      if constexpr (OP == 15) asm volatile("v_pk_add_u16 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 16) asm volatile("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(x[c]) : "v"(y), "v"(z));
      if constexpr (OP == 17) asm volatile("v_mul_lo_u32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      if constexpr (OP == 18) asm volatile("v_fma_f64 %0, %1, %1, %0" : "+v"(dacc[c]) : "v"(dz));
      if constexpr (OP == 19) {  // int32 -> f64, then acc += v * v
        double t;
        asm volatile("v_cvt_f64_i32 %0, %1" : "=v"(t) : "v"(x[c]));
        asm volatile("v_fma_f64 %0, %1, %1, %0" : "+v"(dacc[c]) : "v"(t));
      }
      if constexpr (OP == 20) {
        double t;
        asm volatile("v_cvt_f64_i32 %0, %1" : "=v"(t) : "v"(x[c]));
        x[c] ^= (uint32_t)__builtin_bit_cast(uint64_t, t);
      }
      if constexpr (OP == 21) {  // packed int16 dot: acc += a.lo * b.lo + a.hi * b.hi
        typedef short s2 __attribute__((ext_vector_type(2)));
        x[c] = (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(s2, y), __builtin_bit_cast(s2, z), (int)x[c], false);
      }
      if constexpr (OP == 3) {  // the kernel's mix: 2 bitop3 : 1 bcnt
        x[c] = __builtin_amdgcn_bitop3_b32(x[c], y, z, 0xE8);
        x[c] = __builtin_amdgcn_bitop3_b32(x[c], y, z, 0x96);
        asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(x[c]) : "v"(y));
      }
    }
  }
  uint64_t t1 = __builtin_amdgcn_s_memtime();
  uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  uint32_t acc = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) acc ^= x[c] ^ (uint32_t)__builtin_bit_cast(uint64_t, dacc[c]);
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
  if (threadIdx.x == 0) {
    clk[2 * blockIdx.x] = t1 - t0;
    clk[2 * blockIdx.x + 1] = r1 - r0;
  }
}

template <int OP>
int run(const char* name, int ops_per_chain_iter, int blocks) {
  uint32_t* out;
  uint64_t* clk;
  CHK(hipMalloc(&out, (size_t)blocks * 256 * 4));
  CHK(hipMalloc(&clk, (size_t)blocks * 16));
  hipEvent_t a, b;
  CHK(hipEventCreate(&a));
  CHK(hipEventCreate(&b));
  for (int w = 0; w < 3; ++w) hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, out, clk, 7u);
  CHK(hipEventRecord(a));
  const int reps = 5;
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL(k<OP>, dim3(blocks), dim3(256), 0, 0, out, clk, 7u + r);
  CHK(hipEventRecord(b));
  CHK(hipEventSynchronize(b));
  float ms = 0;
  CHK(hipEventElapsedTime(&ms, a, b));
  uint64_t* h = new uint64_t[2 * blocks];
  CHK(hipMemcpy(h, clk, (size_t)blocks * 16, hipMemcpyDeviceToHost));
  double ratio = 0;
  for (int i = 0; i < blocks; ++i) ratio += (double)h[2 * i] / (double)h[2 * i + 1];
  const double ghz = ratio / blocks * 0.1;  // s_memrealtime ticks at 100 MHz
  const double lane_ops = (double)reps * blocks * 256.0 * ITERS * CH * ops_per_chain_iter;
  const double ops_s = lane_ops / (ms * 1e-3);
  printf("{\"op\": \"%s\", \"blocks\": %d, \"ms\": %.3f, \"lane_ops_per_s\": %.4e, \"clock_ghz\": %.3f, "
         "\"lane_ops_per_clk_per_cu\": %.2f}\n",
         name, blocks, ms / reps, ops_s, ghz, ops_s / (ghz * 1e9) / 256.0);
  delete[] h;
  (void)hipFree(out);
  (void)hipFree(clk);
  return 0;
}

// How much VALU issues beside an int8 MFMA: one wave per SIMD runs independent
// v_mfma_i32_16x16x64_i8 (FORM 16) or v_mfma_i32_32x32x32_i8 (FORM 32) back to back, each
// followed by F independent v_xor_b32.  One FORM-32 instruction is two FORM-16's MACs, so the
// cases to compare are (16, F) twice against (32, 2 F) once.  Cycles from s_memtime.
typedef int hv4i __attribute__((ext_vector_type(4)));
typedef int hv16i __attribute__((ext_vector_type(16)));
constexpr int HOLD_ITERS = 2048, HOLD_U = 8;  // MFMAs per loop body

template <int FORM, int F>
__global__ __launch_bounds__(256) void hold_k(uint32_t* out, uint64_t* clk, uint32_t seed) {
  constexpr int NX = 8;
  uint32_t x[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) x[c] = seed * (threadIdx.x + 1) + c * 0x9E3779B9u;
  const uint32_t y = seed ^ threadIdx.x;
  const hv4i a = {(int)y, (int)(y * 3), (int)(y * 5), (int)(y * 7)}, b = {(int)seed, (int)y, 1, 2};
  hv4i c4[4];
  hv16i c16[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) c4[i] = hv4i{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) c16[i][j] = 0;
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < HOLD_ITERS; ++it) {
#pragma unroll
    for (int u = 0; u < HOLD_U; ++u) {
      if constexpr (FORM == 16)
        asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(c4[u & 3]) : "v"(a), "v"(b));
      else
        asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(c16[u & 1]) : "v"(a), "v"(b));
#pragma unroll
      for (int f = 0; f < F; ++f) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(x[(u * F + f) % NX]) : "v"(y));
    }
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  uint32_t acc = 0;
#pragma unroll
  for (int c = 0; c < NX; ++c) acc ^= x[c];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc ^= (uint32_t)(c4[i][0] ^ c4[i][3]);
#pragma unroll
  for (int i = 0; i < 2; ++i) acc ^= (uint32_t)(c16[i][0] ^ c16[i][15]);
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
  if (threadIdx.x == 0) clk[blockIdx.x] = t1 - t0;
}

template <int FORM, int F>
int run_hold(double* cyc_out) {
  const int blocks = 256;  // one workgroup per CU: one wave per SIMD
  uint32_t* out;
  uint64_t* clk;
  CHK(hipMalloc(&out, (size_t)blocks * 256 * 4));
  CHK(hipMalloc(&clk, (size_t)blocks * 8));
  for (int w = 0; w < 3; ++w) hipLaunchKernelGGL((hold_k<FORM, F>), dim3(blocks), dim3(256), 0, 0, out, clk, 7u + w);
  CHK(hipDeviceSynchronize());
  uint64_t* h = new uint64_t[blocks];
  CHK(hipMemcpy(h, clk, (size_t)blocks * 8, hipMemcpyDeviceToHost));
  double sum = 0;
  for (int i = 0; i < blocks; ++i) sum += (double)h[i];
  const double per_mfma = sum / blocks / ((double)HOLD_ITERS * HOLD_U);
  const double macs = FORM == 16 ? 16.0 * 16 * 64 : 32.0 * 32 * 32;
  printf("{\"op\": \"mfma_hold\", \"form\": \"%s\", \"valu_per_mfma\": %d, \"cycles_per_mfma\": %.2f, "
         "\"cycles_per_16k_macs\": %.2f, \"valu_per_16k_macs\": %.1f}\n",
         FORM == 16 ? "v_mfma_i32_16x16x64_i8" : "v_mfma_i32_32x32x32_i8", F, per_mfma, per_mfma * 16384.0 / macs,
         F * 16384.0 / macs);
  *cyc_out = per_mfma;
  delete[] h;
  (void)hipFree(out);
  (void)hipFree(clk);
  return 0;
}

// VALU ops per MFMA that still issue within 3 % of the bare MFMA's cycles
static int hidden(const int* f, const double* c, int n) {
  int best = 0;
  for (int i = 0; i < n; ++i)
    if (c[i] <= 1.03 * c[0]) best = f[i];
  return best;
}

int run_hold_all() {
  static const int f16[] = {0, 1, 2, 3, 4, 6}, f32[] = {0, 2, 4, 5, 6, 7, 8, 12};
  double c16[6], c32[8];
  if (run_hold<16, 0>(&c16[0]) || run_hold<16, 1>(&c16[1]) || run_hold<16, 2>(&c16[2]) ||
      run_hold<16, 3>(&c16[3]) || run_hold<16, 4>(&c16[4]) || run_hold<16, 6>(&c16[5]))
    return 1;
  if (run_hold<32, 0>(&c32[0]) || run_hold<32, 2>(&c32[1]) || run_hold<32, 4>(&c32[2]) ||
      run_hold<32, 5>(&c32[3]) || run_hold<32, 6>(&c32[4]) || run_hold<32, 7>(&c32[5]) ||
      run_hold<32, 8>(&c32[6]) || run_hold<32, 12>(&c32[7]))
    return 1;
  const int h16 = hidden(f16, c16, 6), h32 = hidden(f32, c32, 8);
  printf("{\"op\": \"mfma_hold_summary\", \"cycles_16x16x64\": %.2f, \"cycles_32x32x32\": %.2f, "
         "\"valu_hidden_16x16x64\": %d, \"valu_hidden_32x32x32\": %d, \"valu_hidden_per_16k_macs\": [%d, %d]}\n",
         c16[0], c32[0], h16, h32, h16, h32 / 2);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--mfma-hold")) return run_hold_all();
  const int blocks = 256 * 8;  // 8 workgroups (32 waves) per CU
  run<0>("v_bitop3_b32", 1, blocks);
  run<1>("v_bcnt_u32_b32", 1, blocks);
  run<2>("v_xor_b32", 1, blocks);
  run<3>("mix_2bitop3_1bcnt", 3, blocks);
  run<0>("v_bitop3_b32@2wps", 1, 256 * 2);
  run<4>("v_xor_b32_e64", 1, blocks);
  run<5>("v_add3_u32", 1, blocks);
  run<6>("v_or3_b32", 1, blocks);
  run<7>("bcnt+xor_e32", 2, blocks);
  run<8>("v_add_u32_e32", 1, blocks);
  run<9>("v_and_b32_e32", 1, blocks);
  run<10>("v_mad_i64_i32(+2 xor/shift)", 1, blocks);
  run<11>("v_mul_i32_i24", 1, blocks);
  run<12>("v_mul_hi_i32_i24", 1, blocks);
  run<13>("v_lshl_add_u32", 1, blocks);
  run<14>("v_perm_b32", 1, blocks);
  run<15>("v_pk_add_u16", 1, blocks);
  run<16>("v_mad_u32_u24", 1, blocks);
  run<17>("v_mul_lo_u32", 1, blocks);
  run<18>("v_fma_f64", 1, blocks);
  run<19>("v_cvt_f64_i32+v_fma_f64", 2, blocks);
  run<20>("v_cvt_f64_i32(+xor)", 1, blocks);
  run<21>("v_dot2_i32_i16", 1, blocks);
  run<2>("v_xor_b32@1wps", 1, 256);
  run<2>("v_xor_b32@2wps", 1, 512);
  run<2>("v_xor_b32@4wps", 1, 1024);
  return 0;
}
