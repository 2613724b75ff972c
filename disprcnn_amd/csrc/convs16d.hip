// convs16d.hip -- 3x3x3 STRIDE-2 convolution (+BN, +ReLU) in split-f16 arithmetic on the f16 matrix cores (gfx950 / CDNA4), round 5.
//
//   reference: hourglass conv1 / conv3, stackhourglass.py:9-12,17-19 (convbn_3d k3 s2 p1 + ReLU), fp32 (config/defaults.py:22).
//
// The arithmetic, the RS16 tensor layout, the K split over the workgroup's waves and the publish / finalize pipeline are those of
// convs16.hip (read its header first).  What differs:
//   * output voxel o reads input 2o + k - 1: a B fragment's 32 lanes read every second voxel of the staged rows (lane base
//     (2*row*SXI + 2*col) * 16 B, the tap (kh, kw) is still a uniform immediate), the slab of one input plane is 2*rows + 1 input rows x
//     2*WT + 2 columns;
//   * depth: output plane zo takes input planes 2zo-1 (kd 0), 2zo (kd 1), 2zo+1 (kd 2).  The walk is over INPUT planes: an even plane
//     (9 taps, 27 MFMAs) feeds one accumulator, an odd plane (18 taps, 54 MFMAs) finishes it and opens the next; a pair of planes = one
//     output plane = 81 MFMAs per wave, published after the odd step and finalized in the shadow of the next even step's MFMAs.
//   * no residual (the reference's stride-2 layers have none).
//   * the columns of a workgroup are ONE stream of steps, as in convs16.hip: the slab ring runs RING - 1 planes ahead into the next
//     column(s), the even step of a column's plane 0 finalizes the LAST plane of the previous column (its base, its lane mask; the
//     exchange buffer and the accumulator alternate with the FLAT output-plane index: Do may be odd), one cold start before the first
//     column and one drain step after the last.  The odd step of a column's last plane runs only its kd = 2 taps (there is no plane Do
//     for the kd = 0 taps to open, and the other accumulator must be clear for the next column).  Same products, same order of
//     summation as the column-by-column walk: bit-identical outputs.
//   * DEI (de-interleaved slab rows): a tap reads every second staged voxel, i.e. 16-byte LDS slots at a stride of two -- 14 lanes on 8 of the
//     16 slots of a bank row, a 2-way conflict whatever the lane order (42-59 % of these kernels' LDS cycles, profiles/r5_pmc.md at 5429fbb).
//     The LDS-DMA lanes therefore gather a staged row as [even columns | odd columns] (each lane's global address is its own), so that tap
//     kw of output column x is position x (kw 0), HALF + x (kw 1), x + 1 (kw 2): unit stride (4 x 7 tiles: rows padded from 16 to 20
//     slots).  Measured (tools/experiments/exp_s16_forms.py, us per launch): 32 -> 64 on 24x56x56, 64 units: 232 against 256 interleaved.
//   * CS (cout split; cin 32 -> cout 64, the hourglass' conv1): instead of two spatial tiles per workgroup and one workgroup per cout tile
//     (the input staged -- and, measured, mostly FETCHED -- once per cout tile: 2.9 GB per launch for a 1.65 GB input), the two wave
//     pairs of a workgroup take the two COUT tiles of ONE spatial tile: one staging of a slab half the size (6 instead of 10 LDS-DMA
//     instructions per wave and plane for the same MFMAs), the input read once.  Measured, Config A conv1 at 1024 / 256 units: 549 / 121 us
//     against 609 / 153 us for the form it replaced (two spatial tiles per workgroup, interleaved rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/disprcnn_hip.h"
#include "s16_ovf.h"
#include "s16_tilemap.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

#define GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define S16_WAITCNT(vm, lgkm) (((vm) & 15) | (7 << 4) | ((lgkm) << 8) | (((vm) >> 4) << 14))

namespace {

// slab geometry shared by the kernel and its launcher
template <int KW, int RT, int WT, bool DEI, bool CS>
struct DGeom {
    static constexpr int RPW = CS ? 1 : 4 / KW;             // spatial MFMA tiles per workgroup
    static constexpr int SXI = 2 * WT + 2;                  // staged input columns
    static constexpr int HALF = WT + 1;                     // DEI: positions of the even columns [0, HALF), of the odd ones [HALF, SXI)
    static constexpr int SXL = (DEI && RT == 4) ? SXI + 4 : SXI;      // LDS row stride in voxels
    static constexpr int SROWS = 2 * RPW * RT + 1;          // staged input rows
    // voxels per chunk plane; the row-major forms' idle lanes (28..31) over-read a row further
    static constexpr int PV = DEI ? (SROWS * SXL + 63) / 64 * 64 : ((SROWS + 1) * SXI + 8 + 63) / 64 * 64;
    static constexpr int SLAB = (KW / 2) * 8 * PV * 16;
};

// KW = cin / 16 K slices; RT x WT OUTPUT voxels per MFMA tile (1 x 28, 2 x 14, 4 x 7); RING slots of one input-plane slab; DEI, CS: header
template <int KW, int RT, int WT, int RING, bool DEI, bool CS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void convs16d_kernel(const drc_s16conv_params p) {
    using GM = DGeom<KW, RT, WT, DEI, CS>;
    static_assert(!CS || KW == 2, "the cout split is the two wave pairs of a cin = 32 workgroup");
    constexpr int RPW = GM::RPW;
    constexpr int CBI = KW / 2;
    constexpr int SXI = GM::SXI, HALF = GM::HALF, SXL = GM::SXL;
    constexpr int SROWS = GM::SROWS;
    constexpr int PV = GM::PV;
    constexpr int CPB = PV * 16;
    constexpr int SLAB = CBI * 8 * CPB;
    constexpr int NPI = PV / 64;                // LDS-DMA instructions per chunk plane
    constexpr int NL = CBI * 8 * NPI / 4;       // ... per wave and slab
    static_assert(NL == CBI * 2 * NPI, "DMA split: each wave stages every fourth chunk plane");
    constexpr int OWN = 16 / KW;
    constexpr int XW = 4096;
    constexpr int NS = 2;                       // stores per finalize (RS16 hi, lo)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* ring = lds;
    char* xchg = lds + RING * SLAB;             // [2 parities][4 waves][XW]

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int n_ = lane & 31, g = lane >> 5;
    const S16TileLane tln = s16_tile_lane<RT, WT>(n_, !(p.lo4 & 0x100));   // row-major tile lanes; lo4 bit 8: the conflict-free order of s16_tilemap.h (experiment)
    const int rl = tln.rl, xl = tln.xl;
    const int r = wave / KW, k = wave % KW;     // wave pair / K slice
    const int rs = CS ? 0 : r;                  // spatial tile of the workgroup
    const int n_ct = CS ? 1 : p.cout / 32;      // cout tiles spread over workgroups
    const int ct = CS ? r : (int)((blockIdx.x >> 3) % n_ct);   // cout tiles side by side on one XCD (see convs16.hip) -- CS: inside the workgroup

    // input geometry (p.D, p.H, p.W) -> output (D/2, H/2, W/2)
    const int Di = p.D, Hi = p.H, Wi = p.W;
    const int Do = Di / 2, Ho = Hi / 2, Wo = Wi / 2;
    const int Wpi = Wi + 2, Hpi = Hi + 2;
    const long i_rowB = (long)Wpi * 128, i_planeB = (long)Hpi * i_rowB, i_cbB = (long)(Di + 2) * i_planeB, i_nB = (long)CBI * i_cbB;
    const int Wpo = Wo + 2, Hpo = Ho + 2;
    const long o_rowB = (long)Wpo * 128, o_planeB = (long)Hpo * o_rowB, o_cbB = (long)(Do + 2) * o_planeB, o_nB = (long)(p.cout / 32) * o_cbB;

    f16x8 wh[27], wl[27];
    {
        const char* wb = (const char*)p.w + ((long)(ct * KW + k) * 54) * 1024 + lane * 16;
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            wh[t] = *(const f16x8*)(wb + (t * 2) * 1024);
            wl[t] = *(const f16x8*)(wb + (t * 2 + 1) * 1024);
        }
    }
    float sc[OWN], sh[OWN];
#pragma unroll
    for (int e = 0; e < OWN; ++e) {
        const int reg = k * OWN + e;
        const int co = ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * g;
        sc[e] = p.scale[co];
        sh[e] = p.shift[co];
    }
    // LDS-DMA: instruction id = wave*NL + i -> (cb, chunk, piece of the plane); lane -> staged voxel v = piece*64 + lane -> (row, column)
    unsigned srcoff[NPI];
#pragma unroll
    for (int h = 0; h < NPI; ++h) {
        const int v = h * 64 + lane;
        const int rr0 = v / SXL, pp = v - rr0 * SXL;         // LDS position -> (staged row, position in the row)
        const bool ok = rr0 < SROWS && pp < SXI;
        const int rr = ok ? rr0 : 0;
        const int xx = !ok ? 0 : (DEI ? (pp < HALF ? 2 * pp : 2 * (pp - HALF) + 1) : pp);     // its input column
        srcoff[h] = (unsigned)(rr * i_rowB + xx * 16);
    }
    const unsigned bfrag = (unsigned)(((k >> 1) * 8 + (k & 1) * 2 + g) * CPB + ((2 * (rs * RT + rl)) * SXL + (DEI ? xl : 2 * xl)) * 16);     // hi; lo at + 4*CPB
    // byte offset of tap (kh, kw) from there: a uniform immediate
    auto tapoff = [](int kh, int kw) constexpr { return (kh * SXL + (DEI ? (kw == 1 ? HALF : (kw >> 1)) : kw)) * 16; };
    const __attribute__((address_space(3))) char* ringl = (const __attribute__((address_space(3))) char*)ring;
    typedef const __attribute__((address_space(3))) f16x8 lds_frag;

    const int n_xt = (Wo + WT - 1) / WT, n_yt = (Ho + RPW * RT - 1) / (RPW * RT);       // ragged last tiles: lanes outside the map are masked (lane_ok)
    const unsigned xcd = blockIdx.x & 7, qx = (blockIdx.x >> 3) / n_ct, per_xcd = (gridDim.x >> 3) / n_ct;
    const unsigned cols_unit = (unsigned)n_yt * n_xt;
    const float relu_lo = p.relu ? 0.f : -65504.f;
    S16Ovf og;                                        // range guard (s16_ovf.h)
#pragma unroll
    for (int e = 0; e < OWN; ++e) { og.see_raw(sc[e], 3.0e38f); og.see_raw(sh[e], 3.0e38f); }      // a NaN / Inf folded BN parameter

    // ---- the columns of this workgroup, in order (XCD-aware, as in convs16.hip).  The pipeline runs through them WITHOUT draining at a
    // column's end: ONE flat sequence of steps (column, input plane), one cold start before the first, one drain step after the last.
    // The slab cursor runs RING - 1 steps ahead of the MFMA step, into the next column(s); the first even step of a column finalizes the
    // LAST output plane of the previous one.
    struct Col { unsigned n; int y0, x0; bool valid; };
    auto col_of = [&](unsigned it) __attribute__((always_inline)) {
        const unsigned j = it * per_xcd + qx;
        const unsigned nl = j / cols_unit;
        const unsigned rem = j - nl * cols_unit;
        const int yb = (int)(rem / n_xt), xt = (int)(rem - (unsigned)yb * n_xt);
        Col c;
        c.n = nl * 8 + xcd;
        c.valid = c.n < (unsigned)p.N;
        c.y0 = yb * RPW * RT;                                    // output tile origin
        c.x0 = xt * WT;
        return c;
    };
    // output side of a column: the unit's base (the buffer resource is made from it where it is used) and this lane's voxel offset in
    // output plane 0 (padded + 1).  Past the last column: valid = ok = false (all dropped)
    struct Ctx { char* yb; unsigned o16; bool ok, valid; };
    auto ctx_of = [&](const Col& c) __attribute__((always_inline)) {
        Ctx q;
        q.yb = (char*)p.y16 + (long)(c.valid ? c.n : 0u) * o_nB;
        const int yl = c.y0 + rs * RT + rl;
        q.valid = c.valid;
        q.ok = c.valid && tln.ok && yl < Ho && c.x0 + xl < Wo;
        if constexpr (KW == 2)
            q.o16 = (unsigned)((long)ct * o_cbB + o_planeB + (long)(yl + 1) * o_rowB + (long)(k * 2 + g) * (Wpo * 16) + (long)(c.x0 + xl + 1) * 16);
        else
            q.o16 = (unsigned)((long)ct * o_cbB + o_planeB + (long)(yl + 1) * o_rowB + (long)((k >> 1) * 2 + g) * (Wpo * 16) + (long)(c.x0 + xl + 1) * 16 + (k & 1) * 8);
        return q;
    };
    const unsigned lo_off = (unsigned)(4 * Wpo * 16);

    unsigned it_c = 0;                                           // the step's column
    {
        const Col c0 = col_of(0);
        if (!c0.valid) {
            og.flush(p.ovf);
            return;
        }
    }
    Ctx cur = ctx_of(col_of(0)), prev = cur;
    prev.ok = prev.valid = false;
    int zo = 0;                                                  // ... and its output plane

    // ---- slab cursor: staged input rows start at input row 2*y0 - 1 = padded row 2*y0, columns at padded column 2*x0.  stage_next()
    // issues the slab of the cursor's (column, plane) and moves on through the flat sequence -- into the next column at a column's end;
    // past the last column it stays on the last slab (re-loaded into a slot nobody reads: the count of vector-memory instructions per
    // step is fixed)
    auto xcol_of = [&](const Col& c) __attribute__((always_inline)) {
        return (const char*)p.x + (long)c.n * i_nB + (long)(2 * c.y0) * i_rowB + (long)(2 * c.x0) * 16;
    };
    unsigned it_s = 0;
    int pl_s = 0;
    const char* xcol_s = xcol_of(col_of(0));
    auto stage_next = [&](int slot) __attribute__((always_inline)) {
        char* dst = ring + slot * SLAB;
#pragma unroll
        for (int ci = 0; ci < CBI * 2; ++ci) {
            const int cc = ci * 4 + wave;                            // this wave's chunk planes (cb*8 + c): every fourth
            const int cb = cc >> 3, c = cc & 7;
            const char* src = xcol_s + (long)cb * i_cbB + (long)(pl_s + 1) * i_planeB + (long)c * (Wpi * 16);
#pragma unroll
            for (int h = 0; h < NPI; ++h)
                __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + srcoff[h]), LDS_PTR(dst + cc * CPB + h * 1024), 16, 0, 0);
        }
        if (pl_s + 1 < Di) {
            ++pl_s;
        } else {
            const Col c = col_of(it_s + 1);
            if (c.valid) {
                ++it_s;
                pl_s = 0;
                xcol_s = xcol_of(c);
            }
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;

    // ---- the one cold start
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(S16_WAITCNT(63, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int s_ = 0; s_ + 1 < RING; ++s_) stage_next(s_);
    int slot = 0;                                         // ring slot of the current input plane

    // one input plane of column `cur`; A: the parity of the FLAT output-plane index (accumulator and exchange buffer).
    //   ODD = false: plane 2zo, taps kd = 1 into acc[A]; finalizes meanwhile the output plane before it in the flat sequence: zo-1, or at
    //                zo = 0 the LAST plane of `prev`.  COMPUTE = false: the drain step after the last column (`cur` is past the end).
    //   ODD = true : plane 2zo+1, taps kd = 2 into acc[A] (complete: published) and kd = 0 into acc[B] (plane zo+1; not at a column's
    //                last plane: there is no plane Do, and acc[B] must be clear for the next column's plane 0).
    auto step = [&](auto AT, auto ODDT, auto COMPT) __attribute__((always_inline)) {
        constexpr int A = decltype(AT)::value, B = A ^ 1;
        constexpr bool ODD = decltype(ODDT)::value, COMPUTE = decltype(COMPT)::value;
        // the slab of this plane landed: in flight behind it may be the RING-2 younger slabs and the previous step's stores
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(S16_WAITCNT((RING - 2) * NL + (ODD ? NS : 0), 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        {
            int ns = slot + RING - 1; ns = ns >= RING ? ns - RING : ns;
            stage_next(ns);                                  // the slot of the previous plane: free since the barrier
        }
        const __attribute__((address_space(3))) char* sb = ringl + slot * SLAB + bfrag;
        if constexpr (!ODD) {
            // ---- finalize the previous plane (partial sums of the K slices, this wave's couts) in the shadow of the 27 MFMAs
            const bool first = zo == 0;
            const bool ok = first ? prev.ok : cur.ok;        // dropped lanes / the step before the workgroup's first plane: not values of the map
            const unsigned o16 = first ? prev.o16 : cur.o16;
            const int zf = first ? Do - 1 : zo - 1;
            const __amdgpu_buffer_rsrc_t y16r = __builtin_amdgcn_make_buffer_rsrc((void*)(first ? prev.yb : cur.yb), 0, 0x7FFFFF00, 0x00020000);
            f32x4 part[4];
            const char* xb = xchg + B * (4 * XW) + (r * KW) * XW + lane * 16;
            if constexpr (KW == 2) {
                part[0] = *(const f32x4*)(xb + (k * 2) * 1024);
                part[1] = *(const f32x4*)(xb + XW + (k * 2) * 1024);
                part[2] = *(const f32x4*)(xb + (k * 2 + 1) * 1024);
                part[3] = *(const f32x4*)(xb + XW + (k * 2 + 1) * 1024);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) part[q] = *(const f32x4*)(xb + q * XW + k * 1024);
            }
            _Float16 vh[OWN], vl[OWN];
            const unsigned long long og_keep = S16Ovf::lanes(ok);
            auto fin = [&](int e) __attribute__((always_inline)) {
                float s_;
                if constexpr (KW == 2) s_ = part[(e >> 2) * 2][e & 3] + part[(e >> 2) * 2 + 1][e & 3];
                else s_ = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
                float x_ = fmaxf(s_ * sc[e] + sh[e], relu_lo);
                x_ = fminf(x_, 65504.f);
                og.see(x_, og_keep);
                vh[e] = (_Float16)x_;
                vl[e] = (_Float16)(x_ - (float)vh[e]);
            };
            f16x8 bh[2], bl[2];
            if constexpr (COMPUTE) {
                bh[0] = *(lds_frag*)(sb);
                bl[0] = *(lds_frag*)(sb + 4 * CPB);
            }
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                if constexpr (COMPUTE) {
                    const int kh = q / 3, kw = q - kh * 3;
                    if (q + 1 < 9) {
                        const int kh1 = (q + 1) / 3, kw1 = (q + 1) - kh1 * 3;
                        bh[(q + 1) & 1] = *(lds_frag*)(sb + tapoff(kh1, kw1));
                        bl[(q + 1) & 1] = *(lds_frag*)(sb + 4 * CPB + tapoff(kh1, kw1));
                    }
                    const f16x8 h_ = bh[q & 1], l_ = bl[q & 1];
                    const int t1 = 9 + kh * 3 + kw;
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], h_, acc[A], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], l_, acc[A], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t1], h_, acc[A], 0, 0, 0);
                }
                if (q < OWN) fin(q);
                if (q == OWN || (OWN == 8 && q == 8)) {
                    const unsigned po = ok ? (unsigned)((long)zf * o_planeB) : 0x80000000u;
                    if constexpr (KW == 2) {
                        f16x8 hi, lo;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { hi[e] = vh[e]; lo[e] = vl[e]; }
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), y16r, o16 + po, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), y16r, o16 + lo_off + po, 0, 0);
                    } else {
                        f16x4 hi, lo;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { hi[e] = vh[e]; lo[e] = vl[e]; }
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, hi), y16r, o16 + po, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lo), y16r, o16 + lo_off + po, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const bool last = zo + 1 == Do;
            f16x8 bh[2], bl[2];
            bh[0] = *(lds_frag*)(sb);
            bl[0] = *(lds_frag*)(sb + 4 * CPB);
            if (!last) {
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    const int kh = q / 3, kw = q - kh * 3;
                    if (q + 1 < 9) {
                        const int kh1 = (q + 1) / 3, kw1 = (q + 1) - kh1 * 3;
                        bh[(q + 1) & 1] = *(lds_frag*)(sb + tapoff(kh1, kw1));
                        bl[(q + 1) & 1] = *(lds_frag*)(sb + 4 * CPB + tapoff(kh1, kw1));
                    }
                    const f16x8 h_ = bh[q & 1], l_ = bl[q & 1];
                    const int t0 = kh * 3 + kw, t2 = 18 + t0;
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], h_, acc[A], 0, 0, 0);
                    acc[B] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], h_, acc[B], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], l_, acc[A], 0, 0, 0);
                    acc[B] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], l_, acc[B], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t2], h_, acc[A], 0, 0, 0);
                    acc[B] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t0], h_, acc[B], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) {
                    const int kh = q / 3, kw = q - kh * 3;
                    if (q + 1 < 9) {
                        const int kh1 = (q + 1) / 3, kw1 = (q + 1) - kh1 * 3;
                        bh[(q + 1) & 1] = *(lds_frag*)(sb + tapoff(kh1, kw1));
                        bl[(q + 1) & 1] = *(lds_frag*)(sb + 4 * CPB + tapoff(kh1, kw1));
                    }
                    const f16x8 h_ = bh[q & 1], l_ = bl[q & 1];
                    const int t2 = 18 + kh * 3 + kw;
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], h_, acc[A], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], l_, acc[A], 0, 0, 0);
                    acc[A] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t2], h_, acc[A], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // output plane zo complete: publish, clear
            const f32x16 a = acc[A];
            char* xb = xchg + A * (4 * XW) + wave * XW + lane * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(xb + q * 1024) = (f32x4){a[q * 4], a[q * 4 + 1], a[q * 4 + 2], a[q * 4 + 3]};
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[A][e] = 0.f;
            // on to the next output plane of the flat sequence
            if (last) {
                zo = 0;
                prev = cur;
                ++it_c;
                cur = ctx_of(col_of(it_c));
            } else {
                ++zo;
            }
        }
        slot = slot + 1 == RING ? 0 : slot + 1;
    };
    using F = std::false_type;
    using T = std::true_type;
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
#pragma unroll 1
    for (;;) {
        if (!cur.valid) {
            step(I0{}, F{}, F{});                            // drain: finalize the last plane (an even step without MFMAs)
            break;
        }
        step(I0{}, F{}, T{});
        step(I0{}, T{}, T{});
        if (!cur.valid) {
            step(I1{}, F{}, F{});
            break;
        }
        step(I1{}, F{}, T{});
        step(I1{}, T{}, T{});
    }
    og.flush(p.ovf);
}

template <int KW, int RT, int WT, int RING, bool DEI, bool CS>
int launch2(const drc_s16conv_params& p, hipStream_t stream) {
    using GM = DGeom<KW, RT, WT, DEI, CS>;
    constexpr int RPW = GM::RPW;
    constexpr size_t lds = (size_t)RING * GM::SLAB + 2 * 4 * 4096;
    static_assert(lds <= 160 * 1024, "LDS");
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)convs16d_kernel<KW, RT, WT, RING, DEI, CS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    const int Ho = p.H / 2, Wo = p.W / 2;
    const long columns = (long)p.N * ((Ho + RPW * RT - 1) / (RPW * RT)) * ((Wo + WT - 1) / WT);
    const int n_ct = CS ? 1 : p.cout / 32;
    long blocks = 256;                                   // column workers x cout tiles (the tiles of a worker side by side on its XCD)
    while (blocks > 8 * n_ct && blocks / (2 * n_ct) >= columns) blocks /= 2;
    hipLaunchKernelGGL((convs16d_kernel<KW, RT, WT, RING, DEI, CS>), dim3((unsigned)blocks), dim3(256), lds, stream, p);
    return (int)hipGetLastError();
}

// lo4 (unused by the arithmetic of this layer) carries the experiment bits: 0x100 the conflict-free tile lanes of s16_tilemap.h, 0x200 interleaved
// slab rows (no DEI), 0x400 no cout split.  0 = the product forms.
template <int KW, int RT, int WT, int RING, int RING_CS>
int launch(const drc_s16conv_params& p, hipStream_t stream) {
    const bool dei = !(p.lo4 & 0x200);
    // (ring depth: the preferred one where it fits the 160 KiB LDS next to the 32 KiB exchange buffers, else two slots)
    constexpr auto ring_of = [](int want, int slab) constexpr { return (size_t)want * slab + 32768 <= 160 * 1024 ? want : 2; };
    if constexpr (KW == 2) {
        if (p.cout == 64 && !(p.lo4 & 0x400)) {
            constexpr int R1 = ring_of(RING_CS, DGeom<KW, RT, WT, true, true>::SLAB), R0 = ring_of(RING_CS, DGeom<KW, RT, WT, false, true>::SLAB);
            return dei ? launch2<KW, RT, WT, R1, true, true>(p, stream) : launch2<KW, RT, WT, R0, false, true>(p, stream);
        }
    }
    constexpr int R1 = ring_of(RING, DGeom<KW, RT, WT, true, false>::SLAB), R0 = ring_of(RING, DGeom<KW, RT, WT, false, false>::SLAB);
    return dei ? launch2<KW, RT, WT, R1, true, false>(p, stream) : launch2<KW, RT, WT, R0, false, false>(p, stream);
}

}  // namespace

// D, H, W = the INPUT dims (all even); the output is (D/2, H/2, W/2)
extern "C" int drc_conv3d_k3s2_s16_supported(int cin, int cout, int D, int H, int W) {
    if (cin != 32 && cin != 64) return 0;
    if (cout != 32 && cout != 64) return 0;
    if (D <= 0 || H <= 0 || W <= 0 || (D & 1) || (H & 1) || (W & 1)) return 0;
    return 1;       // round 6: any even dims (output width <= 7: 4 x 7 tiles, <= 14: 2 x 14, else 1 x 28; the last tiles masked)
}

extern "C" int drc_conv3d_k3s2_s16_fwd(const drc_s16conv_params* pp, void* stream) {
    if (!pp) return -1;
    const drc_s16conv_params& p = *pp;
    if (!p.x || !p.w || !p.scale || !p.shift || !p.y16) return -1;
    if (p.res || p.y32 || p.left || p.right) return -4;
    if (p.N < 0) return -2;
    if (!drc_conv3d_k3s2_s16_supported(p.cin, p.cout, p.D, p.H, p.W)) return -4;
    if (p.N == 0) return 0;
    const long unit_in = (long)(p.cin / 32) * (p.D + 2) * (p.H + 2) * (p.W + 2) * 128;
    if (unit_in >= 0x7FFFFF00L) return -5;
    hipStream_t s = (hipStream_t)stream;
    const int Wo = p.W / 2;
    // (ring depth by what fits the 160 KiB LDS next to the 32 KiB exchange buffers)
    if (Wo <= 7) return p.cin == 32 ? launch<2, 4, 7, 3, 3>(p, s) : launch<4, 4, 7, 2, 2>(p, s);
    if (Wo <= 14) return p.cin == 32 ? launch<2, 2, 14, 3, 3>(p, s) : launch<4, 2, 14, 2, 2>(p, s);
    return p.cin == 32 ? launch<2, 1, 28, 2, 3>(p, s) : launch<4, 1, 28, 2, 2>(p, s);
}
