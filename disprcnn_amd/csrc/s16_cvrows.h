// s16_cvrows.h -- the cost-volume layer (dres0[0]) of the split-f16 family computed from per-row 2D tap maps (round 8).
//
//   reference arithmetic: the concat cost volume of stackhourglass.py:115-128 folded into convbn_3d 64 -> 32 k3 s1 p1 + ReLU (dres0[0],
//   :63-66,130); fp32 (config/defaults.py:22).  Split-f16 products, RS16 layout, packed weights: convs16.hip (read its header first).
//
// Why.  The layer's virtual input is not a general 3D tensor: its 32 left channels are the same 2D map on every disparity plane (only masked),
// its 32 right channels one 2D map moved by one column per plane.  The layer is linear, so the vertical (kh, channel) contraction is done once
// per image row and every one of the D planes is assembled from it with adds.  With s_j = lo4 + j and L~, R~ the maps zero
// outside [0,H) x [0,W), 18 maps per row (a 3 x 1 vertical conv 32 -> 32 per side and (kd, kw)):
//     A[kd][kw](y, v) = sum_{kh,c} w[o, c,      kd, kh, kw] L~[c, y+kh-1, v]
//     B[kd][kw](y, v) = sum_{kh,c} w[o, 32 + c, kd, kh, kw] R~[c, y+kh-1, v]
//     pre(o, j, y, x) = sum_{kd: 0 <= j+kd-1 < D} sum_{kw} [0 <= x+kw-1 < W] [0 <= x-s_j+kw-kd < W] (A[kd][kw](y, x+kw-1) + B[kd][kw](y, x-s_j+kw-kd))
// the same 27 x 64 products per voxel re-associated: the packed weights are used as they are, and the depth edges, the x edges, the band
// around the mask edge and the fully masked voxels (relu(shift)) all fall out of the two predicates.  MFMAs per row: 18 maps x 18 instead of
// 324 per row AND plane.
//
// One arithmetic, one summation order per output value, whatever kernel, workgroup or wave produces it: both kernels of the family that have a
// cost-volume form (convs16_kernel<4,true,...>: one row per work item; convs16w_kernel<4,true>: two) run s16_cvrows_run below.
//   map value:    kh 0..2 outer, K slice (16 channels) 0..1 inner, each product hi*hi, then lo(act)*hi(w), then hi(act)*lo(w), fp32 accumulate
//   output value: kd 0..2 outer, kw 0..2 inner, acc += (A + B), the sum rounded once; masked terms add +0.
//
// Work item: (unit, ROWS consecutive rows, x tile of 28 columns, group of <= 32 planes).  Per row, four waves:
//   stage    rows y-1..y+1 of L (columns x0-1 .. x0+30) and of R (the columns the tile's planes reach: <= 63, one or two 32-column tiles)
//            by LDS-DMA, issued while the previous row is being assembled;
//   maps     waves 0/1: A maps 0..4 / 4..8, waves 2/3: B maps 0..4 / 4..8 (90 MFMAs per wave and 32-column tile; weights register-resident:
//            5 maps x 3 kh x 2 slices x (hi, lo) = 240 VGPRs), published to LDS as fp32 [map][column][32 couts], 16-byte groups XOR-swizzled
//            by the column so that both the MFMA lanes' writes and the assembling lanes' reads are conflict-free;
//   assemble a half wave owns (plane parity, one of the four 8-cout chunks) x 28 columns.  With one wave per SIMD the loop is bound by the
//            number of instructions it issues, of any kind, so it is written for few of them: the nine left terms x two
//            cout groups are loaded once per row into registers (they do not depend on the plane, only their mask does); per plane 18
//            ds_read_b128 of the right terms, whose five distinct columns move by two from a plane to the wave's next (three offsets and
//            masks are carried over, two computed); a term is fma(A, ok ? 1 : 0, B) -- B of a masked term is read from a zero column, so
//            the masked term is +0 and an unmasked one the rounded A + B, bit for bit what reading both from LDS gave (map values are
//            finite); then the family's epilogue (BN scale / shift, ReLU, clamp with the s16_ovf.h guard, hi / lo split, two 16-byte RS16
//            stores).  The right-side shift is an address offset.  The zero halo is never written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/disprcnn_hip.h"
#include "s16_ovf.h"

namespace s16cv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TX = 28;                  // output columns of a work item
constexpr int PG = 32;                  // planes per work item, at most: TX + PG + 3 <= 64 columns of the right map = two MFMA tiles
constexpr int STG_TILE = 8 * 3 * 32 * 16;       // staged tile: [8 chunks][3 rows][32 columns] x 16 B
constexpr int MAP_B = 32 * 128;                 // one map of a tile: [32 columns][32 couts] fp32
constexpr int MAP_TILE = 9 * MAP_B;
constexpr int STG0 = 0, MAPS0 = 3 * STG_TILE, ZCOL0 = MAPS0 + 3 * MAP_TILE;
constexpr int LDS_BYTES = ZCOL0 + 128;
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
static_assert(ZCOL0 % 64 == 0, "a column's second cout group is its first ^ 32, in the zero column too");

#define S16CV_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define S16CV_WAITCNT(vm, lgkm) (((vm) & 15) | (7 << 4) | ((lgkm) << 8) | (((vm) >> 4) << 14))

// rows [y0, y0 + ROWS) x columns [x0, x0 + 28) x planes [j0, j1) of unit n
struct Task { unsigned n; int y, x0, j0, j1; bool valid; };

template <int ROWS>
__device__ __forceinline__ void s16_cvrows_run(const drc_s16conv_params& p, char* lds) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int xl = lane & 31, hf = lane >> 5;
    const int n_ct = p.cout / 32;
    const int ct = (int)((blockIdx.x >> 3) % n_ct);
    const int D = p.D, H = p.H, W = p.W, lo4 = p.lo4;
    const int Wp = W + 2, Hp = H + 2;
    const long rowB = (long)Wp * 128;
    const long planeB = (long)Hp * rowB;
    const long xcbB = (long)(D + 2) * planeB;
    const long ynB = (long)n_ct * xcbB;
    const long mapnB = planeB;

    // ---- maps phase: this wave's side and its five maps m = kd*3 + kw (waves 1, 3: map 4 again, not published), weights for the lifetime of the workgroup
    const int side = wave >> 1, mlo = (wave & 1) * 4;
    f16x8 wh[5][3][2], wl[5][3][2];
#pragma unroll
    for (int mi = 0; mi < 5; ++mi) {
        const int m = mlo + mi, kd = m / 3, kw = m - kd * 3;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int t = kd * 9 + kh * 3 + kw;
                const char* wb = (const char*)p.w + ((long)(ct * 4 + side * 2 + s) * 54 + t * 2) * 1024 + lane * 16;
                wh[mi][kh][s] = *(const f16x8*)wb;
                wl[mi][kh][s] = *(const f16x8*)(wb + 1024);
            }
    }
    // weights as AGPR values, read by the MFMAs directly (convs16.hip): 44 of the 60 fragments next to the five accumulators
    constexpr int PIN_WH = 14;
#pragma unroll
    for (int mi = 0; mi < 5; ++mi)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                asm volatile("" : "+a"(wl[mi][kh][s]));
                if ((mi * 3 + kh) * 2 + s < PIN_WH) asm volatile("" : "+a"(wh[mi][kh][s]));
            }
    // ---- assembly phase: this half wave's plane parity and 8-cout chunk (s, g): couts 16s + 4g + 8(e>>2) + (e&3), e = 0..7
    const int q8 = wave * 2 + hf, sg = q8 & 3, jpar = wave >> 1;
    const int grp0 = (sg >> 1) * 4 + (sg & 1);        // 16-byte cout groups of a map column: grp0 and grp0 + 2 = grp0 ^ 2, 32 bytes apart by XOR
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int co = ct * 32 + (sg >> 1) * 16 + (sg & 1) * 4 + 8 * (e >> 2) + (e & 3);
        sc[e] = p.scale[co];
        sh[e] = p.shift[co];
    }
    const float relu_lo = p.relu ? 0.f : -65504.f;
    const unsigned lo_off = (unsigned)(4 * Wp * 16);
    // ---- staging: pieces wave*3 + i of a tile, piece = 64 consecutive 16-byte voxels of [chunk][row][column]
    int s_chunk[3], s_row[3], s_col[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int idx = (wave * 3 + i) * 64 + lane;
        s_chunk[i] = idx / 96;
        const int rem = idx - s_chunk[i] * 96;
        s_row[i] = rem >> 5;
        s_col[i] = rem & 31;
    }
    if (threadIdx.x < 8) *(f32x4*)(lds + ZCOL0 + threadIdx.x * 16) = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int n_xt = (W + TX - 1) / TX, n_yt = (H + ROWS - 1) / ROWS, n_pg = (D + PG - 1) / PG;
    const unsigned xcd = blockIdx.x & 7, qx = (blockIdx.x >> 3) / n_ct, per_xcd = (gridDim.x >> 3) / n_ct;
    const unsigned items_unit = (unsigned)n_yt * n_xt * n_pg;
    // the row tasks of this workgroup in order: task index = item * ROWS + row of the item (rows behind the map are skipped)
    auto task_of = [&](unsigned idx) __attribute__((always_inline)) {
        Task t;
        for (;; ++idx) {
            const unsigned it = idx / ROWS, rr = idx - it * ROWS;
            const unsigned j = it * per_xcd + qx;
            const unsigned nl = j / items_unit;
            unsigned rem = j - nl * items_unit;
            const int yb = (int)(rem / (unsigned)(n_xt * n_pg));
            rem -= (unsigned)yb * (n_xt * n_pg);
            const int xt = (int)(rem / (unsigned)n_pg), pg = (int)(rem - (unsigned)xt * n_pg);
            t.n = nl * 8 + xcd;
            t.valid = t.n < (unsigned)p.N;
            t.y = yb * ROWS + (int)rr;
            t.x0 = xt * TX;
            t.j0 = pg * PG;
            t.j1 = t.j0 + PG < D ? t.j0 + PG : D;
            if (!t.valid || t.y < H) break;
        }
        struct R { Task t; unsigned idx; } r = {t, idx};
        return r;
    };
    // right-map columns the task's planes reach: [vlo, vhi] (empty: the whole task is masked), in 32-column tiles
    struct Reach { int vlo, nb; };
    auto reach_of = [&](const Task& t) __attribute__((always_inline)) {
        Reach r;
        int vlo = t.x0 - (lo4 + t.j1 - 1) - 2, vhi = t.x0 + TX + 1 - (lo4 + t.j0);
        vlo = vlo > 0 ? vlo : 0;
        vhi = vhi < W - 1 ? vhi : W - 1;
        r.vlo = vlo;
        r.nb = vhi >= vlo ? ((vhi - vlo) >> 5) + 1 : 0;
        return r;
    };
    auto stage = [&](const Task& t) __attribute__((always_inline)) {
        const Reach rc = reach_of(t);
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.left + (long)t.n * mapnB), 0, 0x7FFFFF00, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.right + (long)t.n * mapnB), 0, 0x7FFFFF00, 0x00020000);
#pragma unroll
        for (int T = 0; T < 3; ++T) {
            if (T > rc.nb) break;
            const int v0 = T == 0 ? t.x0 - 1 : rc.vlo + (T - 1) * 32;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int v = v0 + s_col[i];                    // logical column; the stored halo columns -1 and W are zero, beyond them: offset 0 (zero halo)
                const bool ok = v >= -1 && v <= W;
                const unsigned off = ok ? (unsigned)((long)(t.y + s_row[i]) * rowB + (long)s_chunk[i] * (Wp * 16) + (long)(v + 1) * 16) : 0u;
                char* dst = lds + STG0 + T * STG_TILE + (wave * 3 + i) * 1024;
                if (T == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, S16CV_LDS_PTR(dst), 16, off, 0, 0, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, S16CV_LDS_PTR(dst), 16, off, 0, 0, 0);
            }
        }
    };
    typedef const __attribute__((address_space(3))) f16x8 lds_frag;
    typedef const __attribute__((address_space(3))) f32x4 lds_f4;
    const __attribute__((address_space(3))) char* ldsl = (const __attribute__((address_space(3))) char*)lds;

    auto cur = task_of(0);
    if (!cur.t.valid) return;
    S16Ovf og;
#pragma unroll
    for (int e = 0; e < 8; ++e) { og.see_raw(sc[e], 3.0e38f); og.see_raw(sh[e], 3.0e38f); }
    stage(cur.t);
#pragma unroll 1
    for (;;) {
        const Task t = cur.t;
        const Reach rc = reach_of(t);
        // the staged rows landed (every wave waits for its own pieces); the previous row's assembly is over: the maps may be overwritten
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(S16CV_WAITCNT(0, 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // ---- maps
        const int nt = side ? rc.nb : 1;
#pragma unroll 1
        for (int T = 0; T < nt; ++T) {
            const int tile = side + T;                          // staged tile / map tile: 0 left, 1.. right
            const unsigned fb = (unsigned)(STG0 + tile * STG_TILE + (hf * 96 + xl) * 16);
            f32x16 acc[5];
#pragma unroll
            for (int mi = 0; mi < 5; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][e] = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const f16x8 bh = *(lds_frag*)(ldsl + fb + (s * 2 * 96 + kh * 32) * 16);
                    const f16x8 bl = *(lds_frag*)(ldsl + fb + ((4 + s * 2) * 96 + kh * 32) * 16);
#pragma unroll
                    for (int mi = 0; mi < 5; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[mi][kh][s], bh, acc[mi], 0, 0, 0);
#pragma unroll
                    for (int mi = 0; mi < 5; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[mi][kh][s], bl, acc[mi], 0, 0, 0);
#pragma unroll
                    for (int mi = 0; mi < 5; ++mi) acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[mi][kh][s], bh, acc[mi], 0, 0, 0);
                }
            // accumulator registers 4q..4q+3 of lane (column xl, half hf) = couts 8q + 4hf + 0..3 = 16-byte group 2q + hf of the column
#pragma unroll
            for (int mi = 0; mi < 5; ++mi) {
                if (mi == 0 && mlo != 0) continue;
                char* mb = lds + MAPS0 + tile * MAP_TILE + (mlo + mi) * MAP_B + xl * 128;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *(f32x4*)(mb + (((2 * q + hf) ^ (xl & 7)) * 16)) = (f32x4){acc[mi][q * 4], acc[mi][q * 4 + 1], acc[mi][q * 4 + 2], acc[mi][q * 4 + 3]};
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(S16CV_WAITCNT(63, 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // ---- the next row's staging in the shadow of this row's assembly (the staged tiles are free since the barrier)
        const auto nxt = task_of(cur.idx + 1);
        if (nxt.t.valid) stage(nxt.t);
        // ---- assembly
        const int x = t.x0 + xl;
        const bool lane_ok = xl < TX && x < W;
        const unsigned long long og_keep = S16Ovf::lanes(lane_ok);
        const __amdgpu_buffer_rsrc_t y16r = __builtin_amdgcn_make_buffer_rsrc((char*)p.y16 + (long)t.n * ynB, 0, 0x7FFFFF00, 0x00020000);
        const unsigned o16 = (unsigned)((long)ct * xcbB + planeB + (long)(t.y + 1) * rowB + (long)sg * (Wp * 16) + (long)(x + 1) * 16);
        // byte offset of cout group grp0 of column c (0..31) inside a map: the 16-byte groups are XOR-swizzled by the column
        auto col_off = [&](unsigned c) __attribute__((always_inline)) { return c * 128u + (((unsigned)grp0 ^ (c & 7u)) << 4); };
        // the left terms A[kd][kw](y, x + kw - 1): once per row.  A term whose column is outside the map holds the zero column
        bool okA[3];
        f32x4 ar0[9], ar1[9];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int cA = x + kw - 1;
            okA[kw] = lane_ok && cA >= 0 && cA < W;
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const int kw = m % 3;
            const unsigned oa = okA[kw] ? (unsigned)MAPS0 + col_off((unsigned)(xl + kw) & 31u) : (unsigned)(ZCOL0 - m * MAP_B);
            ar0[m] = *(lds_f4*)(ldsl + oa + m * MAP_B);
            ar1[m] = *(lds_f4*)(ldsl + (oa ^ 32u) + m * MAP_B);
        }
        // the right column u + (kw - kd), u = x - s_j, takes five values u - 2 .. u + 2: offset (tile, column, swizzled group) and mask of each
        auto off_of = [&](int cB) __attribute__((always_inline)) {
            const int ib = cB - rc.vlo;
            return (unsigned)(MAPS0 + MAP_TILE) + (unsigned)(ib >> 5) * (unsigned)MAP_TILE + col_off((unsigned)ib & 31u);
        };
        unsigned offB[5];
        bool okB[5];
        const int jb = t.j0 + jpar;
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const int cB = x - (lo4 + jb) + d - 2;
            offB[d] = off_of(cB);
            okB[d] = (unsigned)cB < (unsigned)W;
        }
#pragma unroll 1
        for (int j = jb; j < t.j1; j += 2) {
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
            f32x4 B0[9], B1[9];
            float msk[9];
            auto read = [&](int kd) __attribute__((always_inline)) {
                const bool kd_ok = j + kd - 1 >= 0 && j + kd - 1 < D;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int m = kd * 3 + kw, d = kw - kd + 2;
                    const bool ok = okA[kw] && kd_ok && okB[d];
                    const unsigned ob = ok ? offB[d] : (unsigned)(ZCOL0 - m * MAP_B);
                    B0[m] = *(lds_f4*)(ldsl + ob + m * MAP_B);
                    B1[m] = *(lds_f4*)(ldsl + (ob ^ 32u) + m * MAP_B);
                    msk[m] = ok ? 1.f : 0.f;
                }
            };
            auto add = [&](int kd) __attribute__((always_inline)) {          // kw inner: acc += (A + B), or += +0
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int m = kd * 3 + kw;
                    const f32x4 k = {msk[m], msk[m], msk[m], msk[m]};
                    a0 += __builtin_elementwise_fma(ar0[m], k, B0[m]);
                    a1 += __builtin_elementwise_fma(ar1[m], k, B1[m]);
                }
            };
            // one wait per kd instead of one per term
#pragma unroll
            for (int kd = 0; kd < 3; ++kd) {
                read(kd);
                __builtin_amdgcn_s_waitcnt(S16CV_WAITCNT(63, 0));
                __builtin_amdgcn_sched_barrier(0);
                add(kd);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the wave's next plane j + 2: the right columns move by two
            offB[4] = offB[2]; offB[3] = offB[1]; offB[2] = offB[0];
            okB[4] = okB[2]; okB[3] = okB[1]; okB[2] = okB[0];
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int cB = x - (lo4 + j + 2) + d - 2;
                offB[d] = off_of(cB);
                okB[d] = (unsigned)cB < (unsigned)W;
            }
            f16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s_ = e < 4 ? a0[e & 3] : a1[e & 3];
                float x_ = s_ * sc[e] + sh[e];
                x_ = __builtin_amdgcn_fmed3f(x_, relu_lo, 65504.f);
                og.see(x_, og_keep);
                hi[e] = (_Float16)x_;
                lo[e] = (_Float16)(x_ - (float)hi[e]);
            }
            const unsigned po = lane_ok ? (unsigned)((long)j * planeB) : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), y16r, o16 + po, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), y16r, o16 + lo_off + po, 0, 0);
        }
        if (!nxt.t.valid) break;
        cur = nxt;
    }
    og.flush(p.ovf);
}

// blocks of a launch: one per CU, a multiple of 8 x cout tiles (every XCD runs the same number), fewer where the launch has few work items
template <int ROWS>
inline long s16_cvrows_blocks(const drc_s16conv_params& p) {
    const long items = (long)p.N * ((p.H + ROWS - 1) / ROWS) * ((p.W + TX - 1) / TX) * ((p.D + PG - 1) / PG);
    const int n_ct = p.cout / 32;
    long blocks = 256;
    while (blocks > 8 * n_ct && blocks / (2 * n_ct) >= items) blocks /= 2;
    return blocks;
}

}  // namespace s16cv
