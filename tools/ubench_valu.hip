// Issue-rate microbenchmark for the VALU instruction classes the shading step uses (gfx950):
// cycles per wave-instruction, one wave per SIMD and five waves per SIMD.
//   hipcc --offload-arch=gfx950 -O3 -o ubench_valu tools/ubench_valu.hip && ./ubench_valu
// The last two rows are the node visit's slab arithmetic (csrc/srt_slab.h) as it stands in the path-pool kernel, 23
// instructions a visit, each visit's first plane depending on the verdict of the one before: the min/max form (6 FMAs, 6
// min/max, then max3 / max / min3 / min, the tolerance and the two comparisons) and the sign form (12 FMAs, the same tail).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

#define REP16(x) x x x x x x x x x x x x x x x x

// one node visit's slab test on planes p0..p5 (a box's min and max), near = t6, t1, t3 and far = t0, t2, t4 into the tail
#define VISIT_TAIL \
  "v_max3_f32 %[t6], %[t6], %[t1], %[t3]\n"  /* lo */                   \
  "v_max_f32 %[t6], %[t6], %[tmin]\n"                                    \
  "v_min3_f32 %[t0], %[t0], %[t2], %[t4]\n"  /* hi */                   \
  "v_min_f32 %[t0], %[t0], %[tmax]\n"                                    \
  "v_sub_f32 %[t1], %[t0], %[t6]\n"                                      \
  "v_add_f32_e64 %[t2], |%[t0]|, |%[t6]|\n"                               \
  "v_fma_f32 %[t2], %[k], %[t2], %[tol]\n"                               \
  "v_cmp_ngt_f32_e64 %[un], |%[t1]|, %[t2]\n"                             \
  "v_cmp_gt_f32 vcc, %[t1], %[t2]\n"                                     \
  "v_cndmask_b32 %[t3], %[c0], %[c1], vcc\n"                             \
  "v_add_f32 %[p0], %[p0], %[t3]\n"
#define VISIT_MINMAX                                                      \
  "v_fma_f32 %[t0], %[p0], %[r0], %[m0]\n"                               \
  "v_fma_f32 %[t1], %[p3], %[r0], %[m0]\n"                               \
  "v_fma_f32 %[t2], %[p1], %[r1], %[m1]\n"                               \
  "v_fma_f32 %[t3], %[p4], %[r1], %[m1]\n"                               \
  "v_fma_f32 %[t4], %[p2], %[r2], %[m2]\n"                               \
  "v_fma_f32 %[t5], %[p5], %[r2], %[m2]\n"                               \
  "v_min_f32 %[t6], %[t0], %[t1]\n"                                      \
  "v_max_f32 %[t0], %[t0], %[t1]\n"                                      \
  "v_min_f32 %[t1], %[t2], %[t3]\n"                                      \
  "v_max_f32 %[t2], %[t2], %[t3]\n"                                      \
  "v_min_f32 %[t3], %[t4], %[t5]\n"                                      \
  "v_max_f32 %[t4], %[t4], %[t5]\n" VISIT_TAIL
#define VISIT_SIGN                                                        \
  "v_fma_f32 %[t0], %[p3], %[q0], %[m0]\n"                               \
  "v_fma_f32 %[t1], %[p0], %[q0], %[m0]\n"                               \
  "v_fma_f32 %[t2], %[p4], %[q1], %[m1]\n"                               \
  "v_fma_f32 %[t3], %[p1], %[q1], %[m1]\n"                               \
  "v_fma_f32 %[t4], %[p5], %[q2], %[m2]\n"                               \
  "v_fma_f32 %[t5], %[p2], %[q2], %[m2]\n"                               \
  "v_fma_f32 %[t6], %[p0], %[r0], %[t0]\n"                               \
  "v_fma_f32 %[t0], %[p3], %[r0], %[t1]\n"                               \
  "v_fma_f32 %[t1], %[p1], %[r1], %[t2]\n"                               \
  "v_fma_f32 %[t2], %[p4], %[r1], %[t3]\n"                               \
  "v_fma_f32 %[t3], %[p2], %[r2], %[t4]\n"                               \
  "v_fma_f32 %[t4], %[p5], %[r2], %[t5]\n" VISIT_TAIL
#define VISIT_OPERANDS                                                                                                              \
  : [p0] "+v"(a0), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4), [t5] "=&v"(t5), [t6] "=&v"(t6),  \
    [un] "=&s"(un)                                                                                                                  \
  : [p1] "v"(a1), [p2] "v"(a2), [p3] "v"(a3), [p4] "v"(b1), [p5] "v"(b2), [r0] "v"(r0), [r1] "v"(r1), [r2] "v"(r2), [q0] "v"(q0),   \
    [q1] "v"(q1), [q2] "v"(q2), [m0] "v"(m0), [m1] "v"(m1), [m2] "v"(m2), [tmin] "v"(tmin), [tmax] "v"(tmax), [k] "v"(kk),          \
    [tol] "v"(tol), [c0] "v"(c0), [c1] "v"(c1)                                                                                      \
  : "vcc"
#define VISIT_INSTRUCTIONS 23

template <int OP>
__global__ void k(float* out, int iters, long long* cyc) {
  float a0 = threadIdx.x * 1.0001f + 1.0f, a1 = a0 + 1.0f, a2 = a0 + 2.0f, a3 = a0 + 3.0f;
  uint32_t u0 = threadIdx.x * 2654435761u + 1u, u1 = u0 ^ 0x9e3779b9u, u2 = u0 + 77u, u3 = u0 * 3u;
  double d0 = a0, d1 = a1, d2 = a2, d3 = a3;
  // the visit rows: a box around the origin, a ray through it (r > 0 on x and z, < 0 on y; q = the sign form's other half)
  float b1 = a1 + 4.0f, b2 = a2 + 5.0f, r0 = 0.75f, r1 = 0.0f, r2 = 1.5f, q0 = 0.0f, q1 = -1.25f, q2 = 0.0f, m0 = -0.5f, m1 = 0.25f, m2 = -0.125f;
  float tmin = 0.001f, tmax = 1e30f, kk = 0x1p-21f, tol = 1e-6f, c0 = 0.0f, c1 = 1e-7f, t0, t1, t2, t3, t4, t5, t6;
  unsigned long long un = 0;
  if (OP == 25) r1 = q1;  // the min/max form keeps the reciprocal itself
  long long clk0 = clock64();
  for (int i = 0; i < iters; ++i) {
    if (OP == 25) { REP16(asm volatile(VISIT_MINMAX VISIT_OPERANDS);) }
    if (OP == 26) { REP16(asm volatile(VISIT_SIGN VISIT_OPERANDS);) }
    if (OP == 0) { REP16(asm volatile("v_fma_f32 %0, %0, %1, %2\n v_fma_f32 %1, %1, %2, %3\n v_fma_f32 %2, %2, %3, %0\n v_fma_f32 %3, %3, %0, %1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 1) { REP16(asm volatile("v_mul_lo_u32 %0, %0, %1\n v_mul_lo_u32 %1, %1, %2\n v_mul_lo_u32 %2, %2, %3\n v_mul_lo_u32 %3, %3, %0" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));) }
    if (OP == 2) { REP16(asm volatile("v_mul_hi_u32 %0, %0, %1\n v_mul_hi_u32 %1, %1, %2\n v_mul_hi_u32 %2, %2, %3\n v_mul_hi_u32 %3, %3, %0" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));) }
    if (OP == 3) { REP16(asm volatile("v_fma_f64 %0, %0, %1, %2\n v_fma_f64 %1, %1, %2, %3\n v_fma_f64 %2, %2, %3, %0\n v_fma_f64 %3, %3, %0, %1" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));) }
    if (OP == 4) { REP16(asm volatile("v_rcp_f32 %0, %0\n v_rcp_f32 %1, %1\n v_rcp_f32 %2, %2\n v_rcp_f32 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 5) { REP16(asm volatile("v_sqrt_f32 %0, %0\n v_sqrt_f32 %1, %1\n v_sqrt_f32 %2, %2\n v_sqrt_f32 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 6) { REP16(asm volatile("v_mul_u32_u24 %0, %0, %1\n v_mul_u32_u24 %1, %1, %2\n v_mul_u32_u24 %2, %2, %3\n v_mul_u32_u24 %3, %3, %0" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));) }
    if (OP == 7) { REP16(asm volatile("v_xor_b32 %0, %0, %1\n v_lshlrev_b32 %1, 13, %1\n v_alignbit_b32 %2, %2, %3, 7\n v_add_u32 %3, %3, %0" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));) }
    if (OP == 8) { REP16(asm volatile("v_div_scale_f32 %0, vcc, %0, %1, %0\n v_div_fmas_f32 %1, %1, %2, %3\n v_div_fixup_f32 %2, %2, %3, %0\n v_cvt_f32_u32 %3, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "vcc");) }
    if (OP == 9) { REP16(asm volatile("v_mul_f64 %0, %0, %1\n v_add_f64 %1, %1, %2\n v_floor_f64 %2, %2\n v_cvt_f64_f32 %3, %4" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a0));) }
    if (OP == 10) { unsigned long long w0 = u0, w1 = u1; REP16(asm volatile("v_mad_u64_u32 %0, vcc, %2, %3, %0\n v_mad_u64_u32 %1, vcc, %3, %2, %1\n v_mad_u64_u32 %0, vcc, %2, %2, %0\n v_mad_u64_u32 %1, vcc, %3, %3, %1" : "+v"(w0), "+v"(w1) : "v"(u2), "v"(u3) : "vcc");) u0 ^= (uint32_t)w0 ^ (uint32_t)(w1 >> 32); }
    if (OP == 11) { REP16(asm volatile("v_pk_fma_f32 %0, %0, %1, %1\n v_pk_fma_f32 %1, %1, %0, %0\n v_pk_fma_f32 %0, %0, %1, %1\n v_pk_fma_f32 %1, %1, %0, %0" : "+v"(d0), "+v"(d1));) }
    if (OP == 13) { REP16(asm volatile("v_min_f32 %0, %0, %1\n v_min_f32 %1, %1, %2\n v_min_f32 %2, %2, %3\n v_min_f32 %3, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 14) { REP16(asm volatile("v_min3_f32 %0, %0, %1, %2\n v_max3_f32 %1, %1, %2, %3\n v_min3_f32 %2, %2, %3, %0\n v_max3_f32 %3, %3, %0, %1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 15) { REP16(asm volatile("v_add_f32 %0, %0, %1\n v_add_f32 %1, %1, %2\n v_add_f32 %2, %2, %3\n v_add_f32 %3, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 16) { REP16(asm volatile("v_mul_f32 %0, %0, %1\n v_mul_f32 %1, %1, %2\n v_mul_f32 %2, %2, %3\n v_mul_f32 %3, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 17) { REP16(asm volatile("v_cmp_lt_f32 vcc, %0, %1\n v_cmp_lt_f32 vcc, %1, %2\n v_cmp_lt_f32 vcc, %2, %3\n v_cmp_lt_f32 vcc, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "vcc");) }
    if (OP == 18) { REP16(asm volatile("v_cndmask_b32 %0, %0, %1, vcc\n v_cndmask_b32 %1, %1, %2, vcc\n v_cndmask_b32 %2, %2, %3, vcc\n v_cndmask_b32 %3, %3, %0, vcc" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "vcc");) }
    if (OP == 19) { REP16(asm volatile("v_add_u32 %0, %0, %1\n v_add_u32 %1, %1, %2\n v_add_u32 %2, %2, %3\n v_add_u32 %3, %3, %0" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));) }
    if (OP == 20) { REP16(asm volatile("v_pk_add_f32 %0, %0, %1\n v_pk_mul_f32 %1, %1, %0\n v_pk_add_f32 %0, %0, %1\n v_pk_mul_f32 %1, %1, %0" : "+v"(d0), "+v"(d1));) }
    if (OP == 21) { REP16(asm volatile("v_fma_f32 %0, %0, %1, %2\n v_min_f32 %1, %1, %2\n v_fma_f32 %2, %2, %3, %0\n v_max_f32 %3, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 22) { REP16(asm volatile("v_fma_f32 %0, %0, %1, %2\n s_nop 0\n v_fma_f32 %1, %1, %2, %3\n s_nop 0\n v_fma_f32 %2, %2, %3, %0\n s_nop 0\n v_fma_f32 %3, %3, %0, %1\n s_nop 0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 23) { REP16(asm volatile("v_med3_f32 %0, %0, %1, %2\n v_med3_f32 %1, %1, %2, %3\n v_med3_f32 %2, %2, %3, %0\n v_med3_f32 %3, %3, %0, %1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));) }
    if (OP == 24) { REP16(asm volatile("v_fma_f32 %0, %4, %1, %2\n v_fma_f32 %1, %4, %2, %3\n v_fma_f32 %2, %4, %3, %0\n v_fma_f32 %3, %4, %0, %1" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "s"(iters));) }
    if (OP == 12) { REP16(asm volatile("v_cndmask_b32 %0, %0, %1, vcc\n v_cmp_lt_f32 vcc, %1, %2\n v_min3_f32 %2, %2, %3, %0\n v_max_f32 %3, %3, %0" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "vcc");) }
  }
  long long clk1 = clock64();
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + (float)(u0 ^ u1 ^ u2 ^ u3) + (float)(d0 + d1 + d2 + d3) + (float)(un & 1);
  if (threadIdx.x == 0) cyc[blockIdx.x] = clk1 - clk0;
}

template <int OP>
void run(const char* name, float* out, long long* cyc, int blocksPerCU, int perBlock = 4) {  // perBlock: instructions per asm block
  const int iters = 2000, cus = 256;
  const int grid = cus * blocksPerCU;
  hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(256), 0, 0, out, 10, cyc);
  hipDeviceSynchronize();
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0);
  hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(256), 0, 0, out, iters, cyc);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  long long h[8]; hipMemcpy(h, cyc, sizeof h, hipMemcpyDeviceToHost);
  const double instr = (double)iters * 16.0 * perBlock;  // per wave
  // SIMD cycles per wave-instruction = wall cycles / (instructions per wave x waves per SIMD)
  printf("%-26s %d wave(s)/SIMD: %6.2f clk/instr per wave (clock64), %6.2f SIMD-cycles/instr (at 2.4 GHz from %.3f ms)\n", name, blocksPerCU,
         (double)h[0] / instr, ms * 1e-3 * 2.4e9 / (instr * blocksPerCU), ms);
}

int main() {
  float* out; long long* cyc;
  hipMalloc(&out, 256 * 8 * 256 * sizeof(float)); hipMalloc(&cyc, 256 * 8 * 8);
  for (int b : {1, 4, 5, 8}) {
#define R(op, name) run<op>(name, out, cyc, b);
    R(13, "v_min_f32") R(14, "v_min3/max3_f32") R(15, "v_add_f32") R(16, "v_mul_f32") R(17, "v_cmp_lt_f32 -> vcc") R(18, "v_cndmask_b32") R(19, "v_add_u32")
    R(20, "v_pk_add/mul_f32") R(21, "fma/min/fma/max") R(22, "v_fma_f32 + s_nop 0") R(23, "v_med3_f32") R(24, "v_fma_f32 (one SGPR operand)")
    R(0, "v_fma_f32") R(12, "cndmask/cmp/min3/max") R(7, "xor/shift/alignbit/add") R(1, "v_mul_lo_u32") R(2, "v_mul_hi_u32") R(10, "v_mad_u64_u32")
    R(6, "v_mul_u32_u24") R(3, "v_fma_f64") R(9, "mul/add/floor/cvt f64") R(4, "v_rcp_f32") R(5, "v_sqrt_f32") R(8, "div_scale/fmas/fixup/cvt") R(11, "v_pk_fma_f32")
    run<25>("visit, min/max form (23)", out, cyc, b, VISIT_INSTRUCTIONS);
    run<26>("visit, sign form (23)", out, cyc, b, VISIT_INSTRUCTIONS);
  }
  return 0;
}
