// convs16u.hip -- ConvTranspose3d(k3, s2, p1, output_padding 1) (+BN, +residual, +ReLU) in split-f16 arithmetic on the f16 matrix cores
// (gfx950 / CDNA4), round 5.
//
//   reference: hourglass conv5 / conv6, stackhourglass.py:22-30,44-49; fp32 (config/defaults.py:22).
//
// Arithmetic and the RS16 layout: convs16.hip (hi + lo fp16 pairs, three v_mfma_f32_32x32x16_f16 per fp32 product, fp32 accumulate).
// o = 2i - 1 + k: an even output has one tap per dimension (k = 1, input i), an odd one two (k = 2 at input i, k = 0 at input i + 1):
// 8 output-parity classes (pz, py, px) with (1+pz)(1+py)(1+px) taps -- 27 in all, each of them used exactly once per input voxel.
// The classes are DISJOINT outputs, so the workgroup's four waves split the CLASSES, not K (no partial sums, no exchange):
//     wave 0: (1,1,1) 8 taps | wave 1: (0,1,1) + (1,0,1) 4 + 4 | wave 2: (1,1,0) + (0,0,1) 4 + 2 | wave 3: (1,0,0) + (0,1,0) + (0,0,0) 2 + 2 + 1
// and every wave multiplies all 64 input channels (4 k-steps of 16): its taps' weights stay in registers (<= 8 taps x 4 x (hi, lo) = 256
// VGPRs).  An MFMA tile is RT x WT INPUT voxels (2 x 14, 4 x 7, 1 x 28); the workgroup walks the input planes of one column: plane zi gives
// output plane 2zi (kd = 1: complete at once), closes 2zi - 1 (kd = 0) and opens 2zi + 1 (kd = 2).  The staged slab is (RT + 1) x (WT + 1)
// voxels (the shifts are {0, +1}^2): one LDS-DMA instruction per 8-channel chunk plane.  A step runs the taps that COMPLETE accumulators
// first; their epilogues (BN, residual, ReLU, hi/lo split, 16-byte stores of whole chunks) issue in the shadow of the taps that open the
// next plane's accumulators.
//
// The columns of a workgroup are ONE stream of steps (as in convs16.hip): the slab ring runs RING - 1 steps ahead into the next column(s),
// the residual requests one step ahead, and step zi = 0 of a column closes the last odd output plane 2 Di - 1 of the PREVIOUS column (through
// that column's bases and lane mask) in the epilogue slot that has nothing of its own to close.  One cold start before the first column,
// one drain step (no MFMA) after the last.  The accumulator / residual-set parity is that of the flat step index (Di may be odd); the
// kd = 0 taps of a column's plane 0 (output plane -1) are not run, so the accumulator they would touch still holds the previous
// column's plane.  Same products, same order of summation as the column-by-column walk: bit-identical outputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/disprcnn_hip.h"
#include "s16_ovf.h"
#include "s16_tilemap.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define S16_WAITCNT(vm, lgkm) (((vm) & 15) | (7 << 4) | ((lgkm) << 8) | (((vm) >> 4) << 14))

namespace {

constexpr int PV = 64;            // voxels per chunk plane of a slab
constexpr int CPB = PV * 16;
constexpr int NCH = 16;           // chunk planes of a slab: 64 input channels
constexpr int SLAB = NCH * CPB;
constexpr int RING = 4;
constexpr int NL = NCH / 4;       // LDS-DMA instructions per wave and slab

// ---- roles: the classes (pz*4 + py*2 + px) a wave owns
struct Role { int n; int cls[3]; };
constexpr Role kRoles[4] = {{1, {7, 0, 0}}, {2, {3, 5, 0}}, {2, {6, 1, 0}}, {3, {4, 2, 0}}};
// per dimension and parity: p = 0: (k 1, shift 0); p = 1: (k 2, shift 0), (k 0, shift 1)
struct UTap { int ci, w, kd, sy, sx, open; };        // class slot of the role, weight tap kd*9+kh*3+kw, kd, in-plane shifts, 1: opens the next plane (kd 2)
struct TapList { int n; UTap t[8]; };
constexpr TapList make_taps(int role) {
    TapList L{};
    // completing taps first (kd 1 of the pz = 0 classes, kd 0 of the pz = 1 classes), then the opening ones (kd 2)
    for (int open = 0; open < 2; ++open)
        for (int ci = 0; ci < kRoles[role].n; ++ci) {
            const int c = kRoles[role].cls[ci], pz = c >> 2, py = (c >> 1) & 1, px = c & 1;
            for (int a = 0; a < 1 + pz; ++a) {
                const int kd = pz ? (a ? 0 : 2) : 1;
                if ((kd == 2) != (open == 1)) continue;
                for (int b = 0; b < 1 + py; ++b)
                    for (int d = 0; d < 1 + px; ++d) {
                        const int kh = py ? (b ? 0 : 2) : 1, kw = px ? (d ? 0 : 2) : 1;
                        L.t[L.n++] = UTap{ci, kd * 9 + kh * 3 + kw, kd, py ? b : 0, px ? d : 0, open};
                    }
            }
        }
    return L;
}

template <int ROLE, int RT, int WT>
__device__ __forceinline__ void body(const drc_s16conv_params& p, char* lds, int wave, int lane) {
    constexpr TapList TL = make_taps(ROLE);
    constexpr Role R = kRoles[ROLE];
    constexpr int NT = TL.n;
    constexpr int NF = R.n;                       // accumulators finished (epilogues) per step
    constexpr int NS = 4 * NF;                    // stores (= residual loads) per step
    constexpr int SXI = WT + 1;
    static_assert((RT + 2) * SXI + 4 <= PV || RT == 1, "slab plane");
    char* ring = lds;
    float* bnlds = (float*)(lds + RING * SLAB);   // [2 g][2: scale, shift][16] floats of this cout tile

    const int n_ = lane & 31, g = lane >> 5;
    const S16TileLane tln = s16_tile_lane<RT, WT>(n_, !(p.lo4 & 0x100));    // row-major tile lanes; lo4 bit 8: the conflict-free order of s16_tilemap.h (experiment)
    const int rl = tln.rl, xl = tln.xl;
    const int n_ct = p.cout / 32;
    const int ct = (int)((blockIdx.x >> 3) % n_ct);   // cout tiles side by side on one XCD (see convs16.hip)
    const int Di = p.D, Hi = p.H, Wi = p.W;
    const int Wpi = Wi + 2, Hpi = Hi + 2;
    const long i_rowB = (long)Wpi * 128, i_planeB = (long)Hpi * i_rowB, i_cbB = (long)(Di + 2) * i_planeB, i_nB = 2 * i_cbB;
    const int Wpo = 2 * Wi + 2, Hpo = 2 * Hi + 2;
    const long o_chunkB = (long)Wpo * 16, o_rowB = 8 * o_chunkB, o_planeB = (long)Hpo * o_rowB, o_cbB = (long)(2 * Di + 2) * o_planeB,
               o_nB = (long)(p.cout / 32) * o_cbB;

    // weights of this role's taps: [ct][k-step 4][tap 27][hi, lo][lane][8]
    f16x8 wh[NT][4], wl[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const char* wb = (const char*)p.w + (((long)(ct * 4 + kk) * 27 + TL.t[t].w) * 2) * 1024 + lane * 16;
            wh[t][kk] = *(const f16x8*)wb;
            wl[t][kk] = *(const f16x8*)(wb + 1024);
        }
    // weights as AGPR values, read by the MFMAs directly (convs16.hip): as many fragments as fit next to the role's 2 * R.n
    // accumulators, less four (with all of them the 1 x 28 form spills a VGPR); lo parts first, then hi
    constexpr int PIN_ = (256 - 32 * R.n) / 4 - 4, PIN = PIN_ < 8 * NT ? PIN_ : 8 * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (t * 4 + kk < PIN) asm volatile("" : "+a"(wl[t][kk]));
            if (4 * NT + t * 4 + kk < PIN) asm volatile("" : "+a"(wh[t][kk]));
        }
    // BN scale / shift of the 16 couts a lane holds (register e <-> cout (e&3) + 8(e>>2) + 4g), via LDS (read back per epilogue)
    if (wave == 0 && lane < 32) {
        const int gg = lane >> 4, e = lane & 15;
        const int co = ct * 32 + (e & 3) + 8 * (e >> 2) + 4 * gg;
        bnlds[gg * 32 + e] = p.scale[co];
        bnlds[gg * 32 + 16 + e] = p.shift[co];
    }
    S16Ovf og;                                        // range guard (s16_ovf.h)
    if (wave == 0) {                                  // a NaN / Inf folded BN parameter (lanes 0..31 cover the tile's 32 couts)
        const int co = ct * 32 + (lane & 31);
        og.see_raw(p.scale[co], 3.0e38f);
        og.see_raw(p.shift[co], 3.0e38f);
    }
    unsigned srcoff;
    {
        const bool ok = lane < (RT + 1) * SXI;
        const int rr = ok ? lane / SXI : 0;
        const int xx = ok ? lane - rr * SXI : 0;
        srcoff = (unsigned)(rr * i_rowB + xx * 16);
    }
    const unsigned bbase = (unsigned)(g * CPB + (rl * SXI + xl) * 16);           // chunk plane (kk>>1)*8 + (kk&1)*2 + g; lo at + 4 planes
    const __attribute__((address_space(3))) char* ringl = (const __attribute__((address_space(3))) char*)ring;
    const __attribute__((address_space(3))) float* bnl = (const __attribute__((address_space(3))) float*)bnlds;
    typedef const __attribute__((address_space(3))) f16x8 lds_frag;
    typedef const __attribute__((address_space(3))) f32x4 lds_f4;

    const int n_xt = (Wi + WT - 1) / WT, n_yt = (Hi + RT - 1) / RT;          // ragged last tiles: lanes outside the map are masked (lane_ok)
    const unsigned xcd = blockIdx.x & 7, qx = (blockIdx.x >> 3) / n_ct, per_xcd = (gridDim.x >> 3) / n_ct;
    const unsigned cols_unit = (unsigned)n_yt * n_xt;
    const float relu_lo = p.relu ? 0.f : -65504.f;

    // ---- the columns of this workgroup, in order (XCD-aware, as in convs16.hip).  The pipeline runs through them WITHOUT draining at a
    // column's end: ONE flat sequence of steps (column, input plane zi), one cold start before the first, one drain step after the last.
    // Three cursors walk it: the slabs (RING - 1 steps ahead), the residual requests (one step ahead) and the MFMA / epilogue step itself.
    struct Col { unsigned n; int y0, x0; bool valid; };
    auto col_of = [&](unsigned it) __attribute__((always_inline)) {
        const unsigned j = it * per_xcd + qx;
        const unsigned nl = j / cols_unit;
        const unsigned rem = j - nl * cols_unit;
        const int yb = (int)(rem / n_xt), xt = (int)(rem - (unsigned)yb * n_xt);
        Col c;
        c.n = nl * 8 + xcd;
        c.valid = c.n < (unsigned)p.N;
        c.y0 = yb * RT;                                          // input tile origin
        c.x0 = xt * WT;
        return c;
    };
    // output side of a column: the unit's bases (buffer resources are made from them where they are used) and this lane's even-corner output
    // voxel (2 yl, 2 (x0 + xl)), chunk (s = 0, g), hi, in output plane 0 (padded + 1).  Past the last column: valid = ok = false (all dropped)
    struct Ctx { char* yb; const char* rb; unsigned o_lane; bool ok, valid; };
    auto ctx_of = [&](const Col& c) __attribute__((always_inline)) {
        Ctx q;
        const long ub = (long)(c.valid ? c.n : 0u) * o_nB + (long)ct * o_cbB;
        q.yb = (char*)p.y16 + ub;
        q.rb = p.res ? (const char*)p.res + ub : (const char*)p.w;
        const int yl = c.y0 + rl;
        q.valid = c.valid;
        q.ok = c.valid && tln.ok && yl < Hi && c.x0 + xl < Wi;
        q.o_lane = (unsigned)(o_planeB + (long)(2 * yl + 1) * o_rowB + (long)g * o_chunkB + (long)(2 * (c.x0 + xl) + 1) * 16);
        return q;
    };
    auto pick = [](bool s, const Ctx& a, const Ctx& b) __attribute__((always_inline)) {
        Ctx q;
        q.yb = s ? a.yb : b.yb;
        q.rb = s ? a.rb : b.rb;
        q.o_lane = s ? a.o_lane : b.o_lane;
        q.ok = s ? a.ok : b.ok;
        q.valid = s ? a.valid : b.valid;
        return q;
    };
    const unsigned nres = p.res ? 0x7FFFFF00u : 0u;

    unsigned it_c = 0;                                           // the step's column
    {
        const Col c0 = col_of(0);
        if (!c0.valid) {
            og.flush(p.ovf);
            return;
        }
    }
    Ctx cur = ctx_of(col_of(0)), nxt = ctx_of(col_of(1)), prev = cur;
    prev.ok = prev.valid = false;
    int zi = 0;                                                  // ... and its input plane

    // ---- slab cursor: staged rows start at input row y0 = padded row y0 + 1, columns at padded column x0 + 1.  stage_next() issues the
    // slab of the cursor's (column, plane) and moves on through the flat sequence -- into the next column at a column's end; past the
    // last column it stays on the last slab (re-loaded into a slot nobody reads: the count of vector-memory instructions per step is fixed)
    auto xcol_of = [&](const Col& c) __attribute__((always_inline)) {
        return (const char*)p.x + (long)c.n * i_nB + (long)(c.y0 + 1) * i_rowB + (long)(c.x0 + 1) * 16;
    };
    unsigned it_s = 0;
    int pl_s = 0;
    const char* xcol_s = xcol_of(col_of(0));
    auto stage_next = [&](int slot) __attribute__((always_inline)) {
        char* dst = ring + slot * SLAB;
#pragma unroll
        for (int ci = 0; ci < NL; ++ci) {
            const int cc = ci * 4 + wave;
            const char* src = xcol_s + (long)(cc >> 3) * i_cbB + (long)(pl_s + 1) * i_planeB + (long)(cc & 7) * (Wpi * 16);
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + srcoff), LDS_PTR(dst + cc * CPB), 16, 0, 0);
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

    f32x16 acc[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    // residual tiles are requested ONE STEP before their use (two register sets by the parity of the FLAT step index).  A step at input
    // plane zi finishes output plane 2 zi of its column (pz = 0 classes, context A) and closes 2 zi - 1 (pz = 1 classes, context B) --
    // at zi = 0 that is the LAST odd plane 2 Di - 1 of the PREVIOUS column: B = that column, its bases, its lanes
    u32x4 resv[2][NF][4];
    auto offsets_of = [&](const Ctx& A, int zoA, const Ctx& B, int zoB, unsigned (&fo)[NF]) __attribute__((always_inline)) {
#pragma unroll
        for (int ci = 0; ci < NF; ++ci) {
            const int c = R.cls[ci], pz = c >> 2, py = (c >> 1) & 1, px = c & 1;
            const bool ok = pz ? B.ok : A.ok;
            const unsigned ol = pz ? B.o_lane : A.o_lane;
            const int zo = pz ? zoB : zoA;
            fo[ci] = ok ? ol + (unsigned)((long)zo * o_planeB + (long)py * o_rowB + px * 16) : 0x80000000u;
        }
    };
    auto request = [&](const Ctx& A, int zoA, const Ctx& B, int zoB, auto ST) __attribute__((always_inline)) {        // -> set ST
        constexpr int S_ = decltype(ST)::value;
        unsigned fo[NF];
        offsets_of(A, zoA, B, zoB, fo);
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)A.rb, 0, nres, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)B.rb, 0, nres, 0x00020000);
#pragma unroll
        for (int ci = 0; ci < NF; ++ci)
#pragma unroll
            for (int q = 0; q < 4; ++q)      // q: (lo?, s): chunks s*2 (+g in o_lane), + 4 for lo
                resv[S_][ci][q] = __builtin_amdgcn_raw_buffer_load_b128((R.cls[ci] >> 2) ? rb : ra, fo[ci] + (unsigned)(((q >> 1) * 4 + (q & 1) * 2) * o_chunkB), 0, 0);
    };
    // ---- the one cold start
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(S16_WAITCNT(63, 0));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    request(cur, 0, prev, 0, std::integral_constant<int, 0>{});
#pragma unroll
    for (int s_ = 0; s_ + 1 < RING; ++s_) stage_next(s_);
    __builtin_amdgcn_s_waitcnt(S16_WAITCNT((RING - 2) * NL, 15));      // plane 0 landed (step 0's own wait counts a previous step's stores)
    int slot = 0;

    // one step of parity P (of the flat step index): input plane zi of column `cur` (COMPUTE); COMPUTE = false: the drain step after the
    // last column (`cur` is past the end: it only closes the last odd output plane of `prev`)
    auto step = [&](auto PT, auto COMPT) __attribute__((always_inline)) {
        constexpr int P = decltype(PT)::value;
        constexpr bool COMPUTE = decltype(COMPT)::value;
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(S16_WAITCNT((RING - 2) * NL + NS, 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool first = zi == 0, last = zi + 1 == Di;
        // output planes finished in this step (their residual tiles were requested one step ago into set P); the next step's go out now
        const Ctx cB = pick(first, prev, cur);
        unsigned fo[NF];
        offsets_of(cur, 2 * zi, cB, first ? 2 * Di - 1 : 2 * zi - 1, fo);
        request(pick(last, nxt, cur), last ? 0 : 2 * zi + 2, cur, 2 * zi + 1, std::integral_constant<int, P ^ 1>{});
        {
            int ns = slot + RING - 1; ns = ns >= RING ? ns - RING : ns;
            stage_next(ns);
        }
        const __amdgpu_buffer_rsrc_t ya = __builtin_amdgcn_make_buffer_rsrc((void*)cur.yb, 0, 0x7FFFFF00, 0x00020000);
        const __amdgpu_buffer_rsrc_t yb_ = __builtin_amdgcn_make_buffer_rsrc((void*)cB.yb, 0, 0x7FFFFF00, 0x00020000);
        const __attribute__((address_space(3))) char* sb = ringl + slot * SLAB + bbase;
        auto run_tap = [&](int t) __attribute__((always_inline)) {
            const UTap u = TL.t[t];
            const int pz = R.cls[u.ci] >> 2;
            const int ai = pz ? (u.open ? (P ^ 1) : P) : 0;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int off = ((kk >> 1) * 8 + (kk & 1) * 2) * CPB + (u.sy * SXI + u.sx) * 16;
                const f16x8 h_ = *(lds_frag*)(sb + off), l_ = *(lds_frag*)(sb + off + 4 * CPB);
                acc[u.ci][ai] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t][kk], h_, acc[u.ci][ai], 0, 0, 0);
                acc[u.ci][ai] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t][kk], l_, acc[u.ci][ai], 0, 0, 0);
                acc[u.ci][ai] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t][kk], h_, acc[u.ci][ai], 0, 0, 0);
            }
        };
        if constexpr (COMPUTE) {
            // the completing taps.  kd = 0 at zi = 0 would feed output plane -1: not run -- acc[.][P] holds the previous column's last odd
            // plane there (opened by its last step's kd = 2 taps; the kd = 0 taps of that plane read the zero halo: nothing to add)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (!TL.t[t].open && !(R.cls[TL.t[t].ci] >> 2)) run_tap(t);
            if (!first) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (!TL.t[t].open && (R.cls[TL.t[t].ci] >> 2)) run_tap(t);
            }
        }
        // this step's residual tiles were requested at the head of the PREVIOUS step: younger are that step's DMAs and stores and this step's
        // requests and DMAs
        __builtin_amdgcn_s_waitcnt(S16_WAITCNT(2 * NL + 2 * NS, 15));
        __builtin_amdgcn_sched_barrier(0);
        // ---- epilogues of the finished accumulators (in the shadow of the opening taps below)
#pragma unroll
        for (int ci = 0; ci < NF; ++ci) {
            const int pz = R.cls[ci] >> 2;
            const int ai = pz ? P : 0;
            const f32x16 a = acc[ci][ai];
            const unsigned long long og_keep = S16Ovf::lanes(fo[ci] != 0x80000000u);      // dropped lanes / planes hold over-read data
            f16x8 hi[2], lo[2];
            float og_mx = 0.f;                                   // largest |stored value| of this accumulator (one compare per accumulator)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f32x4 sc0 = *(lds_f4*)(bnl + g * 32 + s * 8), sc1 = *(lds_f4*)(bnl + g * 32 + s * 8 + 4);
                const f32x4 sh0 = *(lds_f4*)(bnl + g * 32 + 16 + s * 8), sh1 = *(lds_f4*)(bnl + g * 32 + 16 + s * 8 + 4);
                const f16x8 rh = __builtin_bit_cast(f16x8, resv[P][ci][s]), rl_ = __builtin_bit_cast(f16x8, resv[P][ci][2 + s]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float sc_ = e < 4 ? sc0[e & 3] : sc1[e & 3], sh_ = e < 4 ? sh0[e & 3] : sh1[e & 3];
                    float x_ = a[s * 8 + e] * sc_ + sh_;
                    x_ += (float)rh[e] + (float)rl_[e];
                    x_ = __builtin_amdgcn_fmed3f(x_, relu_lo, 65504.f);
                    og_mx = fmaxf(og_mx, __builtin_fabsf(x_));
                    hi[s][e] = (_Float16)x_;
                    lo[s][e] = (_Float16)(x_ - (float)hi[s][e]);
                }
            }
            og.see_max(og_mx, og_keep);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi[s]), pz ? yb_ : ya, fo[ci] + (unsigned)((s * 2) * o_chunkB), 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo[s]), pz ? yb_ : ya, fo[ci] + (unsigned)((4 + s * 2) * o_chunkB), 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ci][ai][e] = 0.f;
        }
        if constexpr (COMPUTE) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (TL.t[t].open) run_tap(t);
        }
        slot = slot + 1 == RING ? 0 : slot + 1;
        // on to the next step of the flat sequence
        if (last) {
            zi = 0;
            prev = cur;
            cur = nxt;
            ++it_c;
            nxt = ctx_of(col_of(it_c + 1));
        } else {
            ++zi;
        }
    };
    using F = std::false_type;
    using T = std::true_type;
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
#pragma unroll 1
    for (;;) {
        if (!cur.valid) {
            step(I0{}, F{});
            break;
        }
        step(I0{}, T{});
        if (!cur.valid) {
            step(I1{}, F{});
            break;
        }
        step(I1{}, T{});
    }
    og.flush(p.ovf);
}

template <int RT, int WT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void convs16u_kernel(const drc_s16conv_params p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wave == 0) body<0, RT, WT>(p, lds, wave, lane);
    else if (wave == 1) body<1, RT, WT>(p, lds, wave, lane);
    else if (wave == 2) body<2, RT, WT>(p, lds, wave, lane);
    else body<3, RT, WT>(p, lds, wave, lane);
}

template <int RT, int WT>
int launch(const drc_s16conv_params& p, hipStream_t stream) {
    constexpr size_t lds = (size_t)RING * SLAB + 1024;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)convs16u_kernel<RT, WT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    const long columns = (long)p.N * ((p.H + RT - 1) / RT) * ((p.W + WT - 1) / WT);
    const int n_ct = p.cout / 32;
    long blocks = 256;                                   // column workers x cout tiles (the tiles of a worker side by side on its XCD)
    while (blocks > 8 * n_ct && blocks / (2 * n_ct) >= columns) blocks /= 2;
    hipLaunchKernelGGL((convs16u_kernel<RT, WT>), dim3((unsigned)blocks), dim3(256), lds, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// D, H, W = the INPUT dims; the output is (2D, 2H, 2W); cin = 64
extern "C" int drc_deconv3d_k3s2_s16_supported(int cin, int cout, int D, int H, int W) {
    if (cin != 64 || (cout != 32 && cout != 64)) return 0;
    if (D <= 0 || H <= 0 || W <= 0) return 0;
    return 1;       // round 6: any input dims (W <= 7: 4 x 7 input tiles, <= 14: 2 x 14, else 1 x 28; the last tiles masked)
}

extern "C" int drc_deconv3d_k3s2_s16_fwd(const drc_s16conv_params* pp, void* stream) {
    if (!pp) return -1;
    const drc_s16conv_params& p = *pp;
    if (!p.x || !p.w || !p.scale || !p.shift || !p.y16) return -1;
    if (p.y32 || p.left || p.right) return -4;
    if (p.N < 0) return -2;
    if (!drc_deconv3d_k3s2_s16_supported(p.cin, p.cout, p.D, p.H, p.W)) return -4;
    if (p.N == 0) return 0;
    const long unit_out = (long)(2 * p.D + 2) * (2 * p.H + 2) * (2 * p.W + 2) * 128;      // one 32-channel block
    if (unit_out >= 0x7FFFFF00L / 2) return -5;
    hipStream_t s = (hipStream_t)stream;
    if (p.W <= 7) return launch<4, 7>(p, s);
    if (p.W <= 14) return launch<2, 14>(p, s);
    return launch<1, 28>(p, s);
}
