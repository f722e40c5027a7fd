// Issue rate of the VALU instructions the ADC scans are made of (wave64, gfx950): cycles per wave-instruction per SIMD at full occupancy.
//   hipcc -O3 --offload-arch=gfx950 tools/probes/valu_rate.hip -o tools/probes/valu_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
template <int OP>
__global__ __launch_bounds__(256) void k(uint32_t* out, int iters, uint32_t seed) {
    uint32_t a[8];
    for (int i = 0; i < 8; ++i) a[i] = seed + threadIdx.x * 977u + i * 131u;
    uint32_t sh = (threadIdx.x & 3) * 8, c = threadIdx.x * 4, sel = 64u << sh;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (OP == 0) asm volatile("v_bfe_u32 %0, %0, %1, 8" : "+v"(a[i]) : "v"(sh));
                else if (OP == 1) asm volatile("v_lshl_add_u32 %0, %0, 7, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 2) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 3) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 4) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[i]) : "v"(c));
                else if (OP == 5) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 6) asm volatile("v_and_b32 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 7) asm volatile("v_lshrrev_b32 %0, 3, %0" : "+v"(a[i]));
                else if (OP == 8) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(*(uint64_t*)&a[i & ~1]) : "v"(*(uint64_t*)&a[(i & ~1)]));
                else if (OP == 9) asm volatile("v_min_u32 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 10) asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "v"(sel), "v"(c));
            }
        }
    }
    uint32_t x = 0;
    for (int i = 0; i < 8; ++i) x ^= a[i];
    if (x == 0x12345u) out[0] = x;
}
// The scans' gather as a chain: LDS address of entry (byte of D, lane's column) in a table of 64-byte rows, then ds_read_b64; the value read is
// the next D.  Eight chains per wave, in blocks of four entries (one asm block each, its own wait inside).  FORM 0: v_bfe_u32 + v_lshl_add_u32 per
// address; 1: v_dot4_u32_u8, every read directly behind its dot4 -- with the s_nop 2 the compiler puts there (a ds_read needs its address three
// wait states after a dot instruction); 2: four dot4s, then the four reads (no nop needed); 3: the reads alone, from a fixed address (the floor).
// Addresses stay inside the 16 KB table: 255 * 64 + 56 + 8 bytes at most.
template <int FORM>
__global__ __launch_bounds__(256) void kchain(uint32_t* out, int iters, uint32_t seed) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[4096];
    for (int i = threadIdx.x; i < 4096; i += 256) tab[i] = (seed + i) * 2654435761u;
    __syncthreads();
    const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)tab;
    const uint32_t sh = (threadIdx.x & 3) * 8, sel = 64u << sh, c = base + (threadIdx.x & 7) * 8;
    uint32_t d[8];
    for (int i = 0; i < 8; ++i) d[i] = seed + threadIdx.x * 977u + i * 131u;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int b = 0; b < 8; b += 4) {
            uint32_t t0, t1, t2, t3;
            uint64_t r0, r1, r2, r3;
            if (FORM == 0)
                asm volatile("v_bfe_u32 %4, %8, %12, 8\n\tv_lshl_add_u32 %4, %4, 6, %13\n\tds_read_b64 %0, %4\n\t"
                             "v_bfe_u32 %5, %9, %12, 8\n\tv_lshl_add_u32 %5, %5, 6, %13\n\tds_read_b64 %1, %5\n\t"
                             "v_bfe_u32 %6, %10, %12, 8\n\tv_lshl_add_u32 %6, %6, 6, %13\n\tds_read_b64 %2, %6\n\t"
                             "v_bfe_u32 %7, %11, %12, 8\n\tv_lshl_add_u32 %7, %7, 6, %13\n\tds_read_b64 %3, %7\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                             : "v"(d[b]), "v"(d[b + 1]), "v"(d[b + 2]), "v"(d[b + 3]), "v"(sh), "v"(c));
            else if (FORM == 1)
                asm volatile("v_dot4_u32_u8 %4, %8, %12, %13\n\ts_nop 2\n\tds_read_b64 %0, %4\n\t"
                             "v_dot4_u32_u8 %5, %9, %12, %13\n\ts_nop 2\n\tds_read_b64 %1, %5\n\t"
                             "v_dot4_u32_u8 %6, %10, %12, %13\n\ts_nop 2\n\tds_read_b64 %2, %6\n\t"
                             "v_dot4_u32_u8 %7, %11, %12, %13\n\ts_nop 2\n\tds_read_b64 %3, %7\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                             : "v"(d[b]), "v"(d[b + 1]), "v"(d[b + 2]), "v"(d[b + 3]), "v"(sel), "v"(c));
            else if (FORM == 2)
                asm volatile("v_dot4_u32_u8 %4, %8, %12, %13\n\tv_dot4_u32_u8 %5, %9, %12, %13\n\t"
                             "v_dot4_u32_u8 %6, %10, %12, %13\n\tv_dot4_u32_u8 %7, %11, %12, %13\n\t"
                             "ds_read_b64 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                             : "v"(d[b]), "v"(d[b + 1]), "v"(d[b + 2]), "v"(d[b + 3]), "v"(sel), "v"(c));
            else
                asm volatile("ds_read_b64 %0, %13\n\tds_read_b64 %1, %13\n\tds_read_b64 %2, %13\n\tds_read_b64 %3, %13\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                             : "v"(d[b]), "v"(d[b + 1]), "v"(d[b + 2]), "v"(d[b + 3]), "v"(sel), "v"(c));
            d[b] = (uint32_t)r0; d[b + 1] = (uint32_t)r1; d[b + 2] = (uint32_t)r2; d[b + 3] = (uint32_t)r3;
        }
    }
    uint32_t x = 0;
    for (int i = 0; i < 8; ++i) x ^= d[i];
    if (x == 0x12345u) out[0] = x;
}
template <int FORM>
int run_chain(const char* name, uint32_t* out) {
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int iters = 4000, grid = 256 * 8;   // 8 workgroups of 4 waves per CU = 8 waves per SIMD (8 x 16 KB of LDS)
    float best = 1e9f, worst = 0.f;
    for (int r = 0; r < 6; ++r) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(kchain<FORM>, dim3(grid), dim3(256), 0, 0, out, iters, 12345u);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r) { best = ms < best ? ms : best; worst = ms > worst ? ms : worst; }
    }
    const double ent_per_simd = (double)iters * 8 * 8;    // 8 entries per iteration and wave, 8 waves per SIMD
    printf("%-28s %.3f .. %.3f ms (5 runs)  %.2f ns per entry per SIMD = %.2f cycles at 2.4 GHz\n", name, best, worst, best * 1e6 / ent_per_simd,
           best * 1e6 / ent_per_simd * 2.4);
    return 0;
}
template <int OP>
int run(const char* name, uint32_t* out) {
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int iters = 4000, grid = 256 * 8;   // 8 workgroups of 4 waves per CU = 8 waves per SIMD
    float best = 1e9f;
    for (int r = 0; r < 4; ++r) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(256), 0, 0, out, iters, 12345u);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r) best = ms < best ? ms : best;
    }
    const double instr_per_simd = (double)iters * 32 * 8;    // 32 instructions per iteration and wave, 8 waves per SIMD
    printf("%-16s %.3f ms  %.2f ns per wave-instruction per SIMD = %.2f cycles at 2.4 GHz (%.2f at 2.1)\n", name, best, best * 1e6 / instr_per_simd, best * 1e6 / instr_per_simd * 2.4,
           best * 1e6 / instr_per_simd * 2.1);
    return 0;
}
int main() {
    uint32_t* out; CHECK(hipMalloc(&out, 64));
    run<5>("v_fma_f32", out); run<2>("v_add_f32", out); run<0>("v_bfe_u32", out); run<1>("v_lshl_add_u32", out); run<3>("v_add_u32", out); run<4>("v_cndmask_b32", out);
    run<6>("v_and_b32", out); run<7>("v_lshrrev_b32", out); run<8>("v_pk_add_f32", out); run<9>("v_min_u32", out);
    run<10>("v_dot4_u32_u8", out); run<0>("v_bfe_u32 (again)", out); run<1>("v_lshl_add_u32 (again)", out); run<10>("v_dot4_u32_u8 (again)", out);
    for (int rep = 0; rep < 2; ++rep) {
        run_chain<0>("bfe + lshl_add + ds_read_b64", out); run_chain<1>("dot4, nop 2, ds_read_b64", out);
        run_chain<2>("4 x dot4, 4 x ds_read_b64", out); run_chain<3>("ds_read_b64 alone", out);
    }
    return 0;
}
