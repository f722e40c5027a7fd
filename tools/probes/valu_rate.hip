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
                else if (OP == 11) asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(a[i]) : "v"(c));
                else if (OP == 12) asm volatile("v_lshl_add_u64 %0, %1, 0, %0" : "+v"(*(uint64_t*)&a[i & ~1]) : "v"(*(uint64_t*)&a[(i & ~1) ^ 2]));
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
// The scans' table sums: eight ds_read_b64 (four 16-bit fields each, every field small enough that no sum of eight carries), one wait, then
// the seven adds that fold them -- FORM 0: two v_pk_add_u16 per entry (one per dword, two interleaved chains, as adc16_sum had them); 1: two
// v_add_u32 per entry; 2: one v_lshl_add_u64 per entry (one chain); 3: the reads and the fold-in alone (the floor).  The sum is folded into the
// row's carried value with one 64-bit xor in every form.  Two rows per iteration, as the main loops run them.  The reads are free of bank
// conflicts (lane l reads the 8 bytes at 8 l + 512 i), so that what differs between the forms is the adds.  `extra_lds` bytes of dynamic LDS
// set the occupancy: none for 8 waves per SIMD, 24 KB per workgroup for 4 (the C4 scan's).
template <int FORM>
__global__ __launch_bounds__(256) void kadds(uint32_t* out, int iters, uint32_t seed) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[4096];
    extern __shared__ uint32_t dyn_[];
    for (int i = threadIdx.x; i < 4096; i += 256) tab[i] = ((seed + i) * 2654435761u) & 0x0fff0fffu;
    __syncthreads();
    const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)tab + (threadIdx.x & 63) * 8;
    uint32_t acc[4] = {seed, threadIdx.x, seed * 3u, threadIdx.x * 5u};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            uint64_t r0, r1, r2, r3, r4, r5, r6, r7;
            asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %8 offset:512\n\tds_read_b64 %2, %8 offset:1024\n\tds_read_b64 %3, %8 offset:1536\n\t"
                         "ds_read_b64 %4, %8 offset:2048\n\tds_read_b64 %5, %8 offset:2560\n\tds_read_b64 %6, %8 offset:3072\n\t"
                         "ds_read_b64 %7, %8 offset:3584\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7) : "v"(base + u * 4096));
            uint32_t l0 = (uint32_t)r0, h0 = (uint32_t)(r0 >> 32);
#define PAIRS_ "v"((uint32_t)r1), "v"((uint32_t)(r1 >> 32)), "v"((uint32_t)r2), "v"((uint32_t)(r2 >> 32)), "v"((uint32_t)r3), "v"((uint32_t)(r3 >> 32)), \
               "v"((uint32_t)r4), "v"((uint32_t)(r4 >> 32)), "v"((uint32_t)r5), "v"((uint32_t)(r5 >> 32)), "v"((uint32_t)r6), "v"((uint32_t)(r6 >> 32)), \
               "v"((uint32_t)r7), "v"((uint32_t)(r7 >> 32))
#define ADD14_(INS) INS " %0, %0, %2\n\t" INS " %1, %1, %3\n\t" INS " %0, %0, %4\n\t" INS " %1, %1, %5\n\t" INS " %0, %0, %6\n\t" INS " %1, %1, %7\n\t" \
                    INS " %0, %0, %8\n\t" INS " %1, %1, %9\n\t" INS " %0, %0, %10\n\t" INS " %1, %1, %11\n\t" INS " %0, %0, %12\n\t" INS " %1, %1, %13\n\t" \
                    INS " %0, %0, %14\n\t" INS " %1, %1, %15"
            if (FORM == 0) asm volatile(ADD14_("v_pk_add_u16") : "+v"(l0), "+v"(h0) : PAIRS_);
            else if (FORM == 1) asm volatile(ADD14_("v_add_u32") : "+v"(l0), "+v"(h0) : PAIRS_);
            else if (FORM == 2) {
                asm volatile("v_lshl_add_u64 %0, %1, 0, %0\n\tv_lshl_add_u64 %0, %2, 0, %0\n\tv_lshl_add_u64 %0, %3, 0, %0\n\tv_lshl_add_u64 %0, %4, 0, %0\n\t"
                             "v_lshl_add_u64 %0, %5, 0, %0\n\tv_lshl_add_u64 %0, %6, 0, %0\n\tv_lshl_add_u64 %0, %7, 0, %0"
                             : "+v"(r0) : "v"(r1), "v"(r2), "v"(r3), "v"(r4), "v"(r5), "v"(r6), "v"(r7));
                l0 = (uint32_t)r0; h0 = (uint32_t)(r0 >> 32);
            }
            acc[u] ^= l0;
            acc[2 + u] ^= h0;
        }
    }
    const uint32_t x = acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
    if (x == 0x12345u) out[0] = x + dyn_[0];
}
template <int FORM>
int run_adds(const char* name, uint32_t* out, int extra_lds) {
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int iters = 4000, grid = 256 * 8;
    float best = 1e9f, worst = 0.f;
    for (int r = 0; r < 6; ++r) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(kadds<FORM>, dim3(grid), dim3(256), extra_lds, 0, out, iters, 12345u);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r) { best = ms < best ? ms : best; worst = ms > worst ? ms : worst; }
    }
    const int wps = extra_lds ? 4 : 8;                            // waves per SIMD resident
    const double rows_per_simd = (double)iters * 2 * 8;           // 2 rows per iteration and wave; 2048 workgroups x 4 waves / (256 CUs x 4 SIMDs) = 8 waves per SIMD in all
    printf("%-34s %d waves/SIMD  %.3f .. %.3f ms (5 runs)  %.2f ns per row of 8 entries per SIMD = %.2f cycles at 2.4 GHz\n", name, wps, best, worst,
           best * 1e6 / rows_per_simd, best * 1e6 / rows_per_simd * 2.4);
    return 0;
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
    // the adds of the 16-bit table sums (profiles/valu_rate_adds.txt)
    run<11>("v_pk_add_u16", out); run<12>("v_lshl_add_u64", out); run<3>("v_add_u32 (again)", out);
    run<11>("v_pk_add_u16 (again)", out); run<12>("v_lshl_add_u64 (again)", out);
    for (int rep = 0; rep < 2; ++rep)
        for (int lds = 0; lds <= 24576; lds += 24576) {
            run_adds<0>("8 reads, 7 x 2 v_pk_add_u16", out, lds); run_adds<1>("8 reads, 7 x 2 v_add_u32", out, lds);
            run_adds<2>("8 reads, 7 x v_lshl_add_u64", out, lds); run_adds<3>("8 reads alone", out, lds);
        }
    return 0;
}
