#ifndef CONVS16_KERNEL      // (first pass; see the second one behind the kernel template)
// convs16.hip -- 3x3x3 stride-1 convolution (+BN, +residual, +ReLU) in SPLIT-f16 arithmetic on the f16 matrix cores (gfx950 / CDNA4), round 5.
//
//   reference arithmetic: convbn_3d k3 s1 p1 of stackhourglass.py:7-51,63-88 (dres0 / dres1 / classif[0], hourglass conv2 / conv4) and, fused
//   into the first layer's loads, the concat cost volume of stackhourglass.py:115-128; fp32 (config/defaults.py:22).
//
// Why.  Rounds 2-4 ran these layers as Winograd F(2^3,3^3) on v_mfma_f32_32x32x2_f32.  That instruction executes at the fp32 VECTOR
// rate (157 TFLOP/s, 1/16 of the f16 MFMA) on the SIMD's vector ALU, where it competes with the Winograd butterflies: 0.48 of that
// peak was the end of the road.  Here every fp32 value v is carried as TWO fp16 numbers, hi = fp16(v) and
// lo = fp16(v - hi), i.e. 22-24 significant bits (the fp32 input itself has 24), and a product is three f16 MFMAs into one fp32
// accumulator:  a*w ~= a_hi*w_hi + a_lo*w_hi + a_hi*w_lo  (the dropped a_lo*w_lo is <= 2^-22 |a*w|).  Each f16 product is exact in
// fp32 (11 x 11 bits) and the accumulation is fp32, so the result carries fp32-class error (measured against fp64 next to the
// fp32 FMA chain: tools/experiments/exp_s16.py) at 3/16 of the fp32-MFMA cost: peak 2.5 PF / 3 = 833 TFLOP/s fp32-equivalent.
// Weights are pre-scaled by a power of two (wexp) so that their lo parts stay normal fp16 numbers; 2^-wexp is folded into `scale`.
// Activations are stored unscaled: a lo part below 2^-14 is a subnormal fp16 (the f16 MFMA does not flush it), absolute error <= 2^-25.
// Range: |activation| <= 65504 (fp16 max); BatchNorm'd PSMNet activations are O(1..100).
//
// Layout "RS16" (row-split-16): halfs [N][C/32][D+2pd][H+2][8 chunks][W+2][8], zero halo of one voxel stored (pd = 1 for volumes, 0 for
// 2D maps).  A 32-channel block of one voxel is 8 chunks of 8 halfs: chunk q = p*4 + s*2 + g, p = 0 hi / 1 lo, (s, g) = the k-step and
// k-group of v_mfma_f32_32x32x16_f16 that consume it, element e <-> channel 4g + 8(2s + (e>>2)) + (e&3).  That is exactly the set of
// couts lane (n, g) of the PRODUCING layer's accumulator holds (C/D map: row = (reg&3) + 8(reg>>2) + 4(lane>>5)), so an epilogue
// stores whole 16-byte chunks and the consumer's B fragment is one 16-byte LDS read: no shuffles on either side.
//
// Kernel.  A = weights (32 couts x 16 k), B = activations (16 k x 32 voxels: one image row of 28, lanes 28..31 idle -- the 32x32x16
// form is 15 % faster than 16x16x32 at peak, which pays for the 12.5 %).  A workgroup of four waves owns 4/KW rows x 28 columns of ALL
// depth planes of one unit ("column") and walks the depth: one slab ((rows + 2) x 30 voxels of one input plane) per step through a
// ring of three LDS slots filled by LDS-DMA two steps ahead.  K is split over KW = cin/16 waves (wave k multiplies 16 input channels),
// so a wave holds ALL 27 taps of its K slice in registers (27 x (hi, lo) x 4 VGPRs = 216) and the input is streamed exactly once:
//   per input plane and wave: 9 B-fragment pairs from LDS (18 ds_read_b128), 81 MFMAs (27 taps x 3 products) into the accumulators of
//   the three output planes the slab touches.  A finished plane's accumulator is exchanged between the K-split waves through LDS
//   (each keeps 16/KW registers = the couts it stores), one barrier per step; BN / residual / ReLU / hi-lo split run in the shadow of
//   the next plane's MFMAs.
// CV = the first layer (the concat cost volume of the left / right RS16 2D feature maps is its virtual input: the 64-channel volume never
// exists).  It does not walk the depth: s16_cvrows.h computes it from per-row 2D tap maps (round 8), one row per work item here,
// two in convs16w.hip, bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/disprcnn_hip.h"
#include "s16_cvrows.h"
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
// s_waitcnt immediate (gfx9 encoding: vmcnt[3:0] | expcnt << 4 | lgkmcnt << 8 | vmcnt[5:4] << 14); the BUILTIN, which the compiler's own
// wait-count pass reads (conv16t.hip)
#define S16_WAITCNT(vm, lgkm) (((vm) & 15) | (7 << 4) | ((lgkm) << 8) | (((vm) >> 4) << 14))

namespace {

constexpr int PV_ROWS = 128;    // voxels per chunk plane of a slab (>= (rows + 2) * SX + the 4 columns lanes 28..31 over-read)
constexpr int PV_FLAT = 192;    // ... of the flat form on 28-column maps (7 stacked rows, the last one up to column 8)
constexpr int RING = 3;
#define CONVS16_KERNEL convs16_kernel
#endif

// RT rows x WT columns of the map make one 32-voxel MFMA tile: 1 x 28 (full-resolution maps, tiles along x), 2 x 14 and 4 x 7 (the
// hourglass' half- and quarter-resolution maps: 28 of 32 lanes busy there as well).
// RES: a residual tensor is added; Y32: the output is the blocked fp32 tensor (cout-1 head's input) instead of RS16.  Template flags, not
// run-time ones: a step issues exactly the loads / stores it needs (the counted waits depend on the numbers) and no dropped ones.
// HEAD (classif[0] of a head; KW == 2, full-resolution tiles): the layer's output is NOT stored.  The 32 -> 1 convolution that follows it
// (classif[2], stackhourglass.py:78-88) is linear, out[o] = sum_t sum_c w1[t][c] a[c][o + off(t)] = sum_t P[t][o + off(t)] with the pointwise
// product P[t][v] = sum_c w1[t][c] a[c][v] -- and a finishing wave holds exactly the B fragment of its 16 channels of a[.][v] (the hi / lo
// halfs it would store).  So each K-slice wave runs three more MFMAs per plane (A = w1's 27 taps as rows, split-f16 like every product
// here), the slice-1 half goes through LDS to the slice-0 wave, which sums the three depth taps over the walk and stores, per SOURCE voxel,
// the nine in-plane partial sums S[kh*3+kw][v] = sum_kd P[kd,kh,kw][z + kd - 1 plane of v] (48-byte slots [N][D][H][W][12] floats: j 0..4
// at 0..4, j 5..8 at 8..11).  drc_head_gather_fwd then adds the nine shifted S values per output voxel (+ the previous head's cost).
// HBM per voxel: 48 B written + 48 read instead of 128 written (blocked fp32) + ~175 read by the stand-alone cout-1 kernel.
// ROWS layout (p.head_rows, W == 28 only: one x tile per row, so the three width taps of an OUTPUT column are held by neighbouring lanes of
// the wave that produced them; run-time and wave-uniform, the 12-float layout above is untouched by it).  The width taps are summed here,
// one-lane whole-wave DPP shifts (x - 1 at lane 0 and x + 1 at lane 63 read zero; the idle lanes 28..31 are zeroed first: lane 31 feeds lane
// 32, lane 28 feeds lane 27), and the slot is float [N][D][H][W][4] = (T0, T1a, T1b, T2) per (source row, OUTPUT column):
//     lane half 0 (j = 0..4):  T0  = (o0[x-1] + o1[x]) + o2[x+1]   (kh = 0)        T1a = o3[x-1] + o4[x]          (kh = 1: kw = 0, 1)
//     lane half 1 (j = 5..8):  T1b = o0[x+1]                       (kh = 1: kw = 2) T2  = (o1[x-1] + o2[x]) + o3[x+1]   (kh = 2)
// in exactly this order of additions in every lane, step kind (the drain's last plane included) and batch position.  Half 1's two values
// move to half 0 (v_permlane32_swap, no arithmetic), whose lanes store the 16-byte slot.  There is NO branch on the layout inside a step (a
// branch splits the tap group's block and its VALU work leaves the shadow of the MFMAs: measured +2.7 %): both layouts run the
// same instructions -- the sums are always computed, the layout selects the data and the offsets of the same two stores (the second one
// is dropped by its offset in the rows layout).  drc_head_gather_rows_fwd adds T0[y-1] + (T1a[y] + T1b[y]) + T2[y+1] of the same column:
// 16 B written + 16 read per voxel.
// FLAT, written RT == 0 (the plain and the residual 32 -> 32 layer on 28-column maps: KW == 2, WT == 28, no Y32; its HEAD form and the
// 64 -> 64 form on 14-column maps are described behind this paragraph): a tile is not an
// image row but 32 CONSECUTIVE voxels of the flattened (unit, row, x) order of a group of G units (p.dil bit 0x4000: G = 1, else 4), so all 32
// MFMA columns of a tile work: 24.5 instead of 28 tiles per 28 x 28 plane.  Column c of a group = tiles 2c (wave pair r = 0) and 2c + 1: 64
// voxels f = 64c .. 64c + 63, f = (n - n0) H W + y W + x; voxels past the group's last unit are masked like the ragged tiles of the row form.
// The slab of a column stacks, at the row form's stride SX, the PADDED rows its voxels touch: from the row above the first voxel's to the row
// below the last one's; at a unit seam the bottom halo row of unit n is at once the top halo row of unit n + 1 (both are stored zeros), followed
// by the first map row of n + 1.  A lane's B-fragment address points at its own voxel's row of the stack, so the uniform tap immediates
// (kh*SX + kw)*16 land on that voxel's true neighbours, and the inner loop is the row form's, instruction for instruction: same sums, same
// order, same bits.  A chunk plane is 192 voxels: from H == 3 on a column touches at most 4 map rows in 2 units = 7 stacked rows, the last one
// read up to column 8 (voxel 188); H == 1 | 2 reach 9 | 8 rows only for a column that starts in the last 7 voxels of a row, and a column
// starts at a multiple of 64 voxels of a group of 28 | 56 | 112 | 224: x = 0, 8, 16, 24 (two units: 7 rows).  Staging and store offsets are
// relative to the column's first unit (at most 3 units further: 32 bits).
// FLAT HEAD (p.head_rows == DRC_HEAD_PLANAR; the kernel is named convs16_headflat_kernel, below): the head arithmetic above on flat tiles.  A column is still a fixed set of voxels walked
// through the depth, so w1h / w1l, head_mfma, pkeep / pbuf / pin and head_update with SC / SB are the row form's; only the store differs.  A flat
// tile is no image row, so the width taps cannot be summed across lanes: the nine depth-summed sums are stored per SOURCE voxel in PLANES,
// float [N][D][9][H W], plane j = kh*3 + kw, element y W + x -- lane half 0 stores j = 0..4, half 1 j = 5..8 (its fifth store dropped by its
// offset, so both halves issue five dword stores: NS = 5), each store of a half 32 consecutive floats = one 128-byte segment; no DPP, no
// permlane, no select on the layout.  The offsets are those of the lane's own voxel (du, y, x of ctx_of), relative to the column's first unit
// like the RS16 stores, so a tile across a unit seam lands in two units' planes.  drc_head_gather_planar_fwd (s16_ops.hip) forms the width and
// row sums of the rows layout in the rows layout's order: the same bits.
// FLAT, KW == 4, WT == 14 (the plain and the residual 64 -> 64 layer on 14-column maps, conv2 of the hourglasses, whose row tiles are
// 2 x 14): all four waves split K, so a workgroup has ONE tile and a column is 32 consecutive voxels f = 32c .. 32c + 31 of a group of G units
// (dil bit 0x4000: G = 1, 0x8000: 8, else 4; the host sets exactly one).  Everything above holds with 32 for 64: two channel blocks are staged
// (chunks 0..15 over the four waves), rows are stacked at SX = 16, and a tile touches at most 4 map rows in 2 units from H == 3 on = 7 stacked
// rows = 112 voxels, inside the row form's chunk plane of 128 (8 rows; H == 2 reaches 8 rows).  The host walks every column of a launch and
// refuses the form where one would need a ninth row or a fourth unit behind its first (s16_flat_half_fits).  The epilogue stores half a chunk
// per wave, the row form's KW == 4 rule.  LDS 3 x 32 + 32 KB and 8 LDS-DMA instructions per wave and slab, as the row form.
template <int KW, bool CV, int RT_ = 1, int WT = 28, bool RES = false, bool Y32 = false, bool HEAD = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void CONVS16_KERNEL(const drc_s16conv_params p) {
    constexpr bool FL = RT_ == 0;               // flat tiles: no rows of the map, 32 consecutive voxels
    constexpr int RT = FL ? 1 : RT_;
    static_assert(!HEAD || (KW == 2 && !CV && RT == 1 && !RES && !Y32), "the fused cout-1 head is a form of the 32 -> 32 full-resolution layer");
    static_assert(!CV || (KW == 4 && RT == 1 && WT == 28 && !RES && !Y32), "the cost-volume form: 64 virtual input channels, full-resolution rows, RS16 output");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if constexpr (CV) {
        s16cv::s16_cvrows_run<1>(p, lds);      // (everything below is the depth walk of the layers whose input is a real tensor)
        return;
    }
    constexpr int TX = WT;                      // output columns per tile
    constexpr int SX = WT + 2;                  // staged columns (TX + halo)
    constexpr int RPW = 4 / KW;                 // MFMA tiles per workgroup (RPW * RT output rows)
    constexpr int CBI = KW / 2;                 // 32-channel input blocks
    constexpr int SROWS = RPW * RT + 2;
    static_assert(RT * WT <= 32, "tile shape");
    static_assert(!FL || (((KW == 2 && WT == 28) || (KW == 4 && WT == 14 && !HEAD)) && !CV && !Y32), "flat tiles: the plain / residual / head 32 -> 32 layer on 28-column maps, 64 -> 64 on 14-column maps");
    constexpr int FV = 32 * RPW;                // flat: voxels per column (one tile per wave set)
    constexpr int PV = FL && KW == 2 ? PV_FLAT : PV_ROWS;  // voxels per chunk plane (flat, 14-column maps: 8 stacked rows of 16 fit the row form's plane)
    constexpr int CPB = PV * 16;                // bytes per chunk plane
    constexpr int NH = PV / 64;                 // 64-voxel pieces of a chunk plane: one LDS-DMA instruction each
    constexpr int SLAB = CBI * 8 * CPB;
    constexpr int NL = CBI * 8 * NH / 4;        // LDS-DMA instructions per wave and slab
    constexpr int OWN = 16 / KW;                // accumulator registers (couts per lane) a wave finishes
    constexpr int XW = 4096;                    // bytes a wave publishes per plane: its 16 accumulator registers
    constexpr int NR = RES ? 2 : 0;             // residual loads per step (hi, lo)
    constexpr bool HP = FL && HEAD;             // the flat head: planar partial sums, five dword stores per step
    constexpr int NS = HP ? 5 : 2;              // stores per step (RS16 hi, lo | blocked fp32 x2 | head slot + fifth value | flat head: planes j = 5g .. 5g + 4)
    static_assert(!(Y32 && (KW != 2 || RES)), "the blocked fp32 output exists for the 32-channel layers without residual");
    static_assert(FL || (RT == 1 ? SROWS * SX + 4 <= PV : (SROWS + 1) * SX + 4 <= PV), "slab plane too small (incl. the rows / columns the idle lanes over-read)");
    char* ring = lds;
    char* xchg = lds + RING * SLAB;             // [2 parities][4 waves][XW]
    char* pbuf = xchg + 2 * 4 * XW;             // HEAD: [2 parities][2 tiles][XW] the K-slice-1 halves of P

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int n_ = lane & 31, g = lane >> 5;
    // this lane's voxel inside the MFMA tile: row-major (lanes >= RT * WT idle).  lo4 bit 8 of a non-CV launch selects the bank-conflict-free
    // order of s16_tilemap.h -- measured slower (its stores are less coalesced, the LDS reads were not the limit): an experiment, not the product
    const S16TileLane tln = s16_tile_lane<RT, WT>(n_, !(p.lo4 & 0x100));
    const int rl = tln.rl, xl = tln.xl;
    const int r = wave / KW, k = wave % KW;     // MFMA tile of the workgroup, K slice
    const int n_ct = p.cout / 32;
    const int ct = (int)((blockIdx.x >> 3) % n_ct);   // cout tile of 32: the tiles of one column set run side by side on ONE XCD (block b -> XCD b % 8), so the
                                                      // input the second tile stages is an L2 hit (as separate grid.y passes the input came from HBM once per tile)

    const int D = p.D, H = p.H, W = p.W;
    const int Wp = W + 2, Hp = H + 2;
    const long rowB = (long)Wp * 128;           // bytes: 8 chunks x Wp x 16
    const long planeB = (long)Hp * rowB;
    const long xcbB = (long)(D + 2) * planeB;
    const long xnB = (long)CBI * xcbB;
    const int cbo = p.cout / 32;
    const long ynB = (long)cbo * xcbB;          // RS16 output / residual: same spatial geometry
    // blocked fp32 output: float[N][cout/16][D+2][H+2][W+2][16]
    const long b_rowB = (long)Wp * 64, b_planeB = (long)Hp * b_rowB, b_cbB = (long)(D + 2) * b_planeB, b_nB = (long)(p.cout / 16) * b_cbB;

    // ---- weights of this wave's K slice: all 27 taps, (hi, lo), registers for the lifetime of the workgroup
    f16x8 wh[27], wl[27];
    {
        const char* wb = (const char*)p.w + ((long)(ct * KW + k) * 54) * 1024 + lane * 16;
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            wh[t] = *(const f16x8*)(wb + (t * 2) * 1024);
            wl[t] = *(const f16x8*)(wb + (t * 2 + 1) * 1024);
        }
    }
    // Where they live: 216 weight registers + B fragments + epilogue do not fit the 256 arch VGPRs, so the allocator spilled
    // fragments to AGPRs and copied each back (four v_accvgpr_read_b32) in front of its MFMA, every step.  An MFMA reads srcA from an AGPR
    // as well: the empty asm below makes 41 fragments (164 registers) AGPR values, next to the 48 accumulator registers (+ 16 of the head's
    // z_); pinning more pushes accumulators out into arch VGPRs and the VALU count up.  No instruction is emitted; the MFMAs stay builtins.
    constexpr int PIN_WH = 14;
#pragma unroll
    for (int t = 0; t < 27; ++t) {
        asm volatile("" : "+a"(wl[t]));
        if (t < PIN_WH) asm volatile("" : "+a"(wh[t]));
    }
    // ---- BN scale / shift of the couts this lane finishes: element e <-> cout ct*32 + 4g + 8*(own slot) + ...
    float sc[OWN], sh[OWN];
#pragma unroll
    for (int e = 0; e < OWN; ++e) {
        const int reg = k * OWN + e;
        const int co = ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * g;
        sc[e] = p.scale[co];
        sh[e] = p.shift[co];
    }
    // ---- HEAD: the 32 -> 1 layer's weights as an A operand, [K slice][hi, lo][lane][8 halfs] (s16.pack_head_weight_s16: MFMA row
    // (r&3) + 8(r>>2) + 4g' = tap (kd = r % 3, j = 5g' + r / 3), so lane half g' of the product holds P[kd][j] in register 3(j - 5g') + kd)
    f16x8 w1h = {}, w1l = {};
    if constexpr (HEAD) {
        const char* wb = (const char*)p.w1 + (long)k * 2048 + lane * 16;
        w1h = *(const f16x8*)wb;
        w1l = *(const f16x8*)(wb + 1024);
    }
    // ---- LDS-DMA geometry (column independent): this wave's instructions id = wave*NL + i -> (cb, chunk, half of the plane)
    int srcrow[2], srcx[2];
    bool srcok[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int v = h * 64 + lane;
        srcok[h] = v < SROWS * SX;
        const int rr = srcok[h] ? v / SX : 0;
        srcrow[h] = rr;
        srcx[h] = srcok[h] ? v - rr * SX : 0;
    }
    const unsigned bfrag0 = (unsigned)(((k >> 1) * 8 + (k & 1) * 2 + g) * CPB);                                      // hi; lo at + 4*CPB
    const unsigned bfrag = bfrag0 + (unsigned)(((r * RT + rl) * SX + xl) * 16);                                      // (flat: per column, Ctx::bf)
    const __attribute__((address_space(3))) char* ringl = (const __attribute__((address_space(3))) char*)ring;
    typedef const __attribute__((address_space(3))) f16x8 lds_frag;

    const int n_xt = (W + TX - 1) / TX, n_yt = (H + RPW * RT - 1) / (RPW * RT);     // ragged last x tile / row tile: lanes outside the map are masked (Ctx::ok)
    // depth walk padded to a multiple of three planes (the accumulator / ring-slot rotation J = t mod 3 must be 0 at every column's first
    // plane): planes D .. Dw-1 are PHANTOM -- staged from the zero halo plane, so they add nothing to plane D-1, and never stored
    const int Dw = (D + 2) / 3 * 3;
    // XCD-aware order: block b runs on XCD b % 8; the 32 blocks of an XCD take 32 consecutive columns of the units n % 8 == xcd, so that the
    // row tiles sharing halo rows meet in one L2
    const unsigned xcd = blockIdx.x & 7, qx = (blockIdx.x >> 3) / n_ct, per_xcd = (gridDim.x >> 3) / n_ct;
    // flat: groups of G units take the place of the units (group gi -> XCD gi % 8), columns of FV flattened voxels that of the row tiles
    const int HW = H * W, Hp1 = H + 1;
    const unsigned G = FL ? ((p.dil & 0x4000) ? 1u : (KW == 4 && (p.dil & 0x8000)) ? 8u : 4u) : 1u;
    const unsigned cols_unit = FL ? (G * (unsigned)HW + (unsigned)(FV - 1)) / (unsigned)FV : (unsigned)n_yt * n_xt;

    // ---- the columns of this workgroup, in order; the pipeline below runs through them WITHOUT draining at a column's end: the first two
    // steps of a column publish / finalize the last planes of the previous one, the last two stage the first slabs of the next one.
    // (flat: n = the unit of the column's first voxel, (y0, x0) = that voxel, rem0 = its index in the unit, lim = voxels from there to the
    // end of the group)
    struct Col { unsigned n; int y0, x0; bool valid; int rem0, lim; };
    auto col_of = [&](unsigned it) __attribute__((always_inline)) {
        const unsigned j = it * per_xcd + qx;
        const unsigned nl = j / cols_unit;
        const unsigned rem = j - nl * cols_unit;
        if constexpr (FL) {
            Col c;
            const unsigned n0 = (nl * 8 + xcd) * G;
            const int gu = n0 < (unsigned)p.N ? (int)((unsigned)p.N - n0 < G ? (unsigned)p.N - n0 : G) : 0;      // units of this group
            const int f0 = (int)rem * FV;
            const int u0 = f0 / HW;
            c.valid = f0 < gu * HW;
            c.n = n0 + (unsigned)u0;
            c.rem0 = f0 - u0 * HW;
            c.lim = gu * HW - f0;
            c.y0 = c.rem0 / WT;
            c.x0 = c.rem0 - c.y0 * WT;
            return c;
        }
        const int yb = (int)(rem / n_xt), xt = (int)(rem - (unsigned)yb * n_xt);
        Col c;
        c.n = nl * 8 + xcd;
        c.valid = c.n < (unsigned)p.N;
        c.y0 = yb * RPW * RT;
        c.x0 = xt * TX;
        c.rem0 = c.lim = 0;
        return c;
    };
    // staging source of a column: the unit's input as a buffer base + this lane's byte offsets of its two staged voxels (h = 0, 1); the
    // plane / channel-block / chunk offset of an instruction is a scalar (soffset)
    struct Src { const char* a; unsigned v0, v1, v2, v3; };
    auto src_of = [&](const Col& c) __attribute__((always_inline)) {
        Src q;
        q.a = (const char*)p.x + (long)c.n * xnB;
        q.v2 = q.v3 = 0u;
        if constexpr (FL) {
            // stacked row rr of the slab = padded row y0 + rr of the first unit, continued behind that unit's bottom halo row (which stands for
            // the next unit's top one) with the next unit's padded rows 1 .. H + 1, and so on; rows below the one under the column's last
            // voxel are not needed: dropped by their offset
            const int el = c.rem0 + (c.lim < FV ? c.lim : FV) - 1;                              // the last voxel, counted from the first unit's origin
            const int du_l = (el >= HW) + (el >= 2 * HW) + (el >= 3 * HW);
            const int rr_last = du_l * Hp1 + (el - du_l * HW) / WT - c.y0 + 2;
            static_assert(NH <= 4, "pieces of a chunk plane");
            unsigned vv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int v = h * 64 + lane;
                const int rr = v / SX, xs = v - rr * SX;
                const int L = c.y0 + rr, M = L - 1;
                const int uo = (M >= Hp1) + (M >= 2 * Hp1) + (M >= 3 * Hp1);
                const unsigned off = (unsigned)((long)uo * xnB + (long)(L - uo * Hp1) * rowB + (long)xs * 16);
                vv[h] = rr <= rr_last ? off : 0x80000000u;
            }
            q.v0 = vv[0]; q.v1 = vv[1]; q.v2 = vv[2]; q.v3 = vv[3];
            return q;
        }
        q.v0 = (unsigned)((long)(c.y0 + srcrow[0]) * rowB + (long)(c.x0 + srcx[0]) * 16);
        q.v1 = (unsigned)((long)(c.y0 + srcrow[1]) * rowB + (long)(c.x0 + srcx[1]) * 16);
        return q;
    };
    auto stage = [&](const Src& q, int pl, int slot) __attribute__((always_inline)) {       // input plane pl of a column -> ring slot
        char* dst = ring + slot * SLAB;
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)q.a, 0, 0x7FFFFF00, 0x00020000);
        const unsigned va[4] = {q.v0, q.v1, q.v2, q.v3};
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int id = wave * NL + i;
            // (flat: NL a multiple of NH -- the piece h of an instruction is a constant, its channel block and chunk wave-uniform)
            const int fc = wave * (NL / NH) + i / NH;
            const int cb = FL ? (CBI == 1 ? 0 : fc >> 3) : id >> 4, c = FL ? (CBI == 1 ? fc : fc & 7) : (id >> 1) & 7, h = FL ? i % NH : id & 1;
            const int so = (int)((long)cb * xcbB + (long)(pl + 1) * planeB + (long)c * (Wp * 16));
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, LDS_PTR(dst + (cb * 8 + c) * CPB + h * 1024), 16, va[h], so, 0, 0);
        }
    };
    // output context of a column: unit bases + this lane's voxel offsets (plane 0, padded coordinates + 1)
    const bool hrows = HEAD && p.head_rows;                                         // the rows layout: float [N][D][H][W][4]
    const int hs_slotB = hrows ? 16 : 48;
    const long hs_planeB = HP ? (long)HW * 36 : (long)H * W * hs_slotB, hs_nB = (long)D * hs_planeB;    // HEAD: float [N][D][H][W][12]; flat: float [N][D][9][H W]
    const unsigned hs_jB = (unsigned)HW * 4u;                                      // flat head: bytes of one of the nine planes of a depth plane
    const bool hs_drop0 = hrows && g, hs_drop1 = hrows || g;                        // lanes whose first / second store is dropped by its offset
    struct Ctx { char* y16b; char* y32b; const char* resb; char* hsb; unsigned o16, o32, ohs, bf; bool ok; };
    auto ctx_of = [&](const Col& c) __attribute__((always_inline)) {
        Ctx q;
        q.bf = bfrag;
        if constexpr (FL) {
            // this lane's voxel: number 32 r + n_ of the column (KW == 4: r == 0), du units behind the column's first one; a lane past the group's end is masked
            // and reads (never stores) the slab's first voxel
            q.hsb = HEAD ? (char*)p.head + (long)c.n * hs_nB : (char*)p.w;
            q.y32b = (char*)p.w;
            q.ohs = q.o32 = 0u;
            q.y16b = HEAD ? (char*)p.w : (char*)p.y16 + (long)c.n * ynB;
            q.resb = p.res ? (const char*)p.res + (long)c.n * ynB : (const char*)p.w;
            q.ok = r * 32 + n_ < c.lim;
            const int e0 = q.ok ? c.rem0 + r * 32 + n_ : c.rem0;
            const int du = (e0 >= HW) + (e0 >= 2 * HW) + (e0 >= 3 * HW);
            const int e = e0 - du * HW;
            const int yl = e / WT, xv = e - yl * WT;
            q.bf = bfrag0 + (unsigned)(((du * Hp1 + yl - c.y0) * SX + xv) * 16);
            // (the row form's rule: KW == 2 a whole chunk per wave, KW == 4 half a chunk)
            const int och = KW == 2 ? k * 2 + g : (k >> 1) * 2 + g, ohalf = KW == 2 ? 0 : (k & 1) * 8;
            q.o16 = (unsigned)((long)du * ynB + (long)ct * xcbB + planeB + (long)(yl + 1) * rowB + (long)och * (Wp * 16) + (long)(xv + 1) * 16 + ohalf);
            // flat head: element y W + x of plane j = 5g of the lane's own voxel (planes 5g + 1 .. at + hs_jB each), relative to the column's first unit
            if constexpr (HEAD) q.ohs = (unsigned)((long)du * hs_nB + (long)(5 * g) * hs_jB + (long)e * 4);
            return q;
        }
        q.hsb = HEAD ? (char*)p.head + (long)c.n * hs_nB : (char*)p.w;
        q.ohs = (unsigned)(((long)(c.y0 + r * RT + rl) * W + (c.x0 + xl)) * hs_slotB + (hrows ? 0 : g * 32));
        q.y16b = p.y16 ? (char*)p.y16 + (long)c.n * ynB : (char*)p.w;
        q.y32b = p.y32 ? (char*)p.y32 + (long)c.n * b_nB : (char*)p.w;
        q.resb = p.res ? (const char*)p.res + (long)c.n * ynB : (const char*)p.w;
        const int yl = c.y0 + r * RT + rl;                                  // this lane's output row
        q.ok = tln.ok && yl < H && c.x0 + xl < W;
        if constexpr (KW == 2) {
            // own registers 8k..8k+7 = chunk (s = k, g) complete: 16 B hi at chunk k*2+g, lo at 4 + k*2 + g
            q.o16 = (unsigned)((long)ct * xcbB + planeB + (long)(yl + 1) * rowB + (long)(k * 2 + g) * (Wp * 16) + (long)(c.x0 + xl + 1) * 16);
            // blocked fp32: block 2ct + k, channels 4g..4g+3 and 8+4g..
            q.o32 = (unsigned)((long)(2 * ct + k) * b_cbB + b_planeB + (long)(yl + 1) * b_rowB + (long)(c.x0 + xl + 1) * 64 + g * 16);
        } else {
            // own registers 4k..4k+3 = couts 8k + 4g + e: half a chunk: chunk (s = k>>1, g), bytes (k&1)*8..
            q.o16 = (unsigned)((long)ct * xcbB + planeB + (long)(yl + 1) * rowB + (long)((k >> 1) * 2 + g) * (Wp * 16) + (long)(c.x0 + xl + 1) * 16 + (k & 1) * 8);
            q.o32 = (unsigned)((long)(2 * ct + (k >> 1)) * b_cbB + b_planeB + (long)(yl + 1) * b_rowB + (long)(c.x0 + xl + 1) * 64 + (k & 1) * 32 + g * 16);
        }
        return q;
    };
    const unsigned lo_off = (unsigned)(4 * Wp * 16);
    const float relu_lo = p.relu ? 0.f : -65504.f;
    const unsigned n16 = p.y16 ? 0x7FFFFF00u : 0u, n32 = p.y32 ? 0x7FFFFF00u : 0u, nres = p.res ? 0x7FFFFF00u : 0u;

    Col ccur = col_of(0);
    if (!ccur.valid) return;
    S16Ovf og;                                              // range guard (s16_ovf.h): a finalized value sat on the clamp, or a folded BN parameter is NaN / Inf
#pragma unroll
    for (int e = 0; e < OWN; ++e) { og.see_raw(sc[e], 3.0e38f); og.see_raw(sh[e], 3.0e38f); }
    Src s_cur = src_of(ccur), s_next = s_cur;
    Ctx cx_cur = ctx_of(ccur), cx_prev = cx_cur;
    cx_prev.ok = false;

    f32x16 acc[3];
    u32x4 resv[3][2];        // residual (hi, lo) tiles, requested a full step before their use: slot J holds the tile requested in a step with t % 3 == J
#pragma unroll
    for (int a_ = 0; a_ < 3; ++a_)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a_][e] = 0.f;
#pragma unroll
    for (int a_ = 0; a_ < 3; ++a_) resv[a_][0] = resv[a_][1] = (u32x4){0u, 0u, 0u, 0u};
    // HEAD: the P of the plane finalized in the previous step (this wave's K slice) and the running depth sums of the two output planes
    // still open (SC: the next to complete; SB: the one after), five (kh, kw) per lane
    f32x16 pkeep = {};
    float SC[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, SB[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // HEAD: what the first store of a step writes from five depth-summed values -- o[0..3] (12-float slots), or in the rows layout the
    // width taps summed across lanes in the order of the header comment.  x - 1: wave_shr:1 (lane i reads lane i - 1), x + 1: wave_shl:1,
    // bound_ctrl: a lane without a source reads zero; v_permlane32_swap(a, b)[1]: lanes 0..31 = a's lanes 32..63
    auto head_pack = [&](const float* o) __attribute__((always_inline)) {
        const bool live = n_ < WT;
        int v_[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) v_[j] = __builtin_bit_cast(int, live ? o[j] : 0.f);
        auto left = [](int a) __attribute__((always_inline)) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, a, 0x138, 0xf, 0xf, true)); };
        auto right = [](int a) __attribute__((always_inline)) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, a, 0x130, 0xf, 0xf, true)); };
        auto own = [](int a) __attribute__((always_inline)) { return __builtin_bit_cast(float, a); };
        const float a0 = (left(v_[0]) + own(v_[1])) + right(v_[2]);         // g = 0: T0
        const float a1 = left(v_[3]) + own(v_[4]);                           // g = 0: T1a
        const float b0 = right(v_[0]);                                       // g = 1: T1b
        const float b1 = (left(v_[1]) + own(v_[2])) + right(v_[3]);         // g = 1: T2
        const unsigned x0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, b0), 0u, false, false)[1];
        const unsigned x1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, b1), 0u, false, false)[1];
        u32x4 d;
        d[0] = hrows ? __builtin_bit_cast(unsigned, a0) : __builtin_bit_cast(unsigned, o[0]);
        d[1] = hrows ? __builtin_bit_cast(unsigned, a1) : __builtin_bit_cast(unsigned, o[1]);
        d[2] = hrows ? x0 : __builtin_bit_cast(unsigned, o[2]);
        d[3] = hrows ? x1 : __builtin_bit_cast(unsigned, o[3]);
        return d;
    };
    stage(s_cur, 0, 0);
    stage(s_cur, 1 < D ? 1 : D, 1);
    __builtin_amdgcn_s_waitcnt(S16_WAITCNT(NL, 15));      // plane 0 landed (step 0's own wait assumes a full previous step)
    unsigned gs = 0;                                       // steps so far: parity of the exchange buffer

    // one step of the pipeline.  KIND 0: input plane t of the current column into the accumulators of output planes t-1, t, t+1;
    // 1: t = 0 (no plane t-1: those taps are skipped); 2: t = D-1 (no plane t+1); 3: drain, no input plane (t = D, D+1 after the last column).
    // Every step publishes output plane t-1 (t = 0: the previous column's plane D-1) and finalizes plane t-2 (t < 2: the previous column's
    // D-2+t).  Straight-line code (no branch between the barrier and the publish): the finalize is spread over the tap groups, so its
    // VALU / LDS / store instructions issue in the shadow of the MFMAs.
    auto step = [&](int t, auto JT, auto KT) __attribute__((always_inline)) {
        constexpr int J = decltype(JT)::value;              // t mod 3 (D % 3 == 0: continuous across columns)
        constexpr int KIND = decltype(KT)::value;
        constexpr bool COMPUTE = KIND != 3;
        constexpr int A0 = (J + 1) % 3, A1 = J, A2 = (J + 2) % 3;    // accumulators of output planes t+1 (kd 0), t (kd 1), t-1 (kd 2)
        // slab t landed (everything but the previous step's requests may be waited for: vmcnt retires in order); lgkmcnt: my exchange
        // writes are visible before the barrier
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(S16_WAITCNT(NL + NS + NR, 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // contexts of the planes finalized / published in this step
        const bool fcur = t >= 2, pcur = t >= 1;
        const int qf = fcur ? t - 2 : Dw - 2 + t, qp = pcur ? t - 1 : Dw - 1;
        const __amdgpu_buffer_rsrc_t resr = __builtin_amdgcn_make_buffer_rsrc((void*)(pcur ? cx_cur.resb : cx_prev.resb), 0, nres, 0x00020000);
        const unsigned p_o16 = pcur ? cx_cur.o16 : cx_prev.o16;
        const bool p_ok = (pcur ? cx_cur.ok : cx_prev.ok) && qp >= 0 && qp < D;
        if constexpr (RES) {
            // the residual of the plane this step PUBLISHES (finalized in the next step): requested now, a whole step before its use
            const unsigned po = p_ok ? (unsigned)((long)qp * planeB) : 0x80000000u;
            if constexpr (KW == 2) {
                resv[J][0] = __builtin_amdgcn_raw_buffer_load_b128(resr, p_o16 + po, 0, 0);
                resv[J][1] = __builtin_amdgcn_raw_buffer_load_b128(resr, p_o16 + lo_off + po, 0, 0);
            } else {
                const u32x2 a_ = __builtin_amdgcn_raw_buffer_load_b64(resr, p_o16 + po, 0, 0);
                const u32x2 b_ = __builtin_amdgcn_raw_buffer_load_b64(resr, p_o16 + lo_off + po, 0, 0);
                resv[J][0] = (u32x4){a_.x, a_.y, 0u, 0u};
                resv[J][1] = (u32x4){b_.x, b_.y, 0u, 0u};
            }
        }
        {   // slab t+2 (of the next column behind this one's last plane) into the slot of plane t-1: free since the barrier
            const int tp = t + 2;
            const bool nxt = tp >= Dw;
            Src q;
            q.a = nxt ? s_next.a : s_cur.a;
            q.v0 = nxt ? s_next.v0 : s_cur.v0;
            q.v1 = nxt ? s_next.v1 : s_cur.v1;
            q.v2 = nxt ? s_next.v2 : s_cur.v2;
            q.v3 = nxt ? s_next.v3 : s_cur.v3;
            int pl = nxt ? tp - Dw : tp;
            pl = pl < D ? pl : D;                       // phantom planes (and the over-staging behind the last column): the zero halo plane D + 1
            stage(q, pl, (J + 2) % 3);
        }
        const __amdgpu_buffer_rsrc_t y16r = __builtin_amdgcn_make_buffer_rsrc(fcur ? cx_cur.y16b : cx_prev.y16b, 0, n16, 0x00020000);
        const __amdgpu_buffer_rsrc_t y32r = __builtin_amdgcn_make_buffer_rsrc(fcur ? cx_cur.y32b : cx_prev.y32b, 0, n32, 0x00020000);
        const unsigned f_o16 = fcur ? cx_cur.o16 : cx_prev.o16, f_o32 = fcur ? cx_cur.o32 : cx_prev.o32;
        const bool f_ok = (fcur ? cx_cur.ok : cx_prev.ok) && qf >= 0 && qf < D;
        // the K-split partial sums of the plane to finalize (published in the previous step), this wave's couts: registers k*OWN .. of
        // every K slice
        f32x4 part[4];
        {
            const char* xb = xchg + ((gs - 1) & 1) * (4 * XW) + (r * KW) * XW + lane * 16;
            if constexpr (KW == 2) {
                part[0] = *(const f32x4*)(xb + (k * 2) * 1024);
                part[1] = *(const f32x4*)(xb + XW + (k * 2) * 1024);
                part[2] = *(const f32x4*)(xb + (k * 2 + 1) * 1024);
                part[3] = *(const f32x4*)(xb + XW + (k * 2 + 1) * 1024);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) part[q] = *(const f32x4*)(xb + q * XW + k * 1024);
            }
        }
        f32x4 pin[4];
        if constexpr (HEAD) {       // the other K slice's half of the P computed in the previous step
            const char* pb = pbuf + ((gs - 1) & 1) * (2 * XW) + r * XW + lane * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) pin[q] = *(const f32x4*)(pb + q * 1024);
        }
        // its residual was requested at the head of the previous step: younger are that step's DMAs and stores and this step's requests
        if constexpr (RES) {
            __builtin_amdgcn_s_waitcnt(S16_WAITCNT(2 * NL + NS + NR, 15));
            __builtin_amdgcn_sched_barrier(0);
        }
        float v[OWN];
        _Float16 vh[OWN], vl[OWN];
        const unsigned long long og_keep = S16Ovf::lanes(f_ok);       // idle lanes / dropped planes hold over-read data: not a value of the map
        auto fin = [&](int e) __attribute__((always_inline)) {
            float s_;
            if constexpr (KW == 2) s_ = part[(e >> 2) * 2][e & 3] + part[(e >> 2) * 2 + 1][e & 3];
            else s_ = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
            float x_ = s_ * sc[e] + sh[e];
            if constexpr (RES) {
                const _Float16 rh = __builtin_bit_cast(f16x8, resv[(J + 2) % 3][0])[e], rl_ = __builtin_bit_cast(f16x8, resv[(J + 2) % 3][1])[e];
                x_ += (float)rh + (float)rl_;
            }
            x_ = __builtin_amdgcn_fmed3f(x_, relu_lo, 65504.f);    // ReLU (relu_lo = 0) or the fp16 range of the hi part (relu_lo = -65504)
            og.see(x_, og_keep);
            v[e] = x_;
            vh[e] = (_Float16)x_;
            vl[e] = (_Float16)(x_ - (float)vh[e]);
        };
        auto stores = [&]() __attribute__((always_inline)) {
            if constexpr (Y32) {
                const unsigned po32 = f_ok ? (unsigned)((long)qf * b_planeB) : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){v[0], v[1], v[2], v[3]}), y32r, f_o32 + po32, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){v[4], v[5], v[6], v[7]}), y32r, f_o32 + 32 + po32, 0, 0);
            } else {
                const unsigned po = f_ok ? (unsigned)((long)qf * planeB) : 0x80000000u;
                if constexpr (KW == 2) {
                    f16x8 hi, lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { hi[e] = vh[e]; lo[e] = vl[e]; }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), y16r, f_o16 + po, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), y16r, f_o16 + lo_off + po, 0, 0);
                } else {
                    f16x4 hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { hi[e] = vh[e]; lo[e] = vl[e]; }
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, hi), y16r, f_o16 + po, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lo), y16r, f_o16 + lo_off + po, 0, 0);
                }
            }
        };
        // output plane t-1 complete: publish the accumulator (every K slice publishes all 16 registers; the finisher of a cout group sums
        // the slices in a fixed order), clear it, request the residual
        auto publish = [&]() __attribute__((always_inline)) {
            const f32x16 a = acc[A2];
            char* xb = xchg + (gs & 1) * (4 * XW) + wave * XW + lane * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(xb + q * 1024) = (f32x4){a[q * 4], a[q * 4 + 1], a[q * 4 + 2], a[q * 4 + 3]};
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[A2][e] = 0.f;
        };
        // HEAD.  (1) The P of the plane finalized in the PREVIOUS step is complete (own K slice in pkeep, the other in pin): source plane
        // s = t - 3 of this column (t < 3: the previous column's D - 3 + t).  It closes output plane s - 1 (kd = 2), adds to plane s (kd = 1) and
        // opens s + 1 (kd = 0); s == 0 (t == 3) instead closes the previous column's last plane and drops what its last source plane opened.
        // One plane is stored per step: this column's t - 4, or the previous one's D - 4 + t.  The five (kh, kw) of a lane are updated one per
        // tap group (head_update(jj) in group jj), the stores go out in group 5.  (2) The P of the plane finalized in THIS step from the hi / lo
        // halfs just computed: three MFMAs between those of the last tap group (head_mfma).
        float o_[5];
        f32x16 z_ = {};
        f16x8 bh_ = {}, bl_ = {};
        auto head_update = [&](int jj) __attribute__((always_inline)) {
            if constexpr (HEAD) {
                const bool first = t == 3;
                const float p0 = pkeep[3 * jj] + pin[(3 * jj) >> 2][(3 * jj) & 3];
                const float p1 = pkeep[3 * jj + 1] + pin[(3 * jj + 1) >> 2][(3 * jj + 1) & 3];
                const float p2 = pkeep[3 * jj + 2] + pin[(3 * jj + 2) >> 2][(3 * jj + 2) & 3];
                o_[jj] = SC[jj] + (first ? 0.f : p2);
                SC[jj] = (first ? 0.f : SB[jj]) + p1;
                SB[jj] = p0;
            }
        };
        auto head_store = [&]() __attribute__((always_inline)) {
            if constexpr (HEAD) {
                const bool scur = t >= 4;
                const int ps = scur ? t - 4 : Dw - 4 + t;
                const bool ok_ = k == 0 && (scur ? cx_cur.ok : cx_prev.ok) && ps >= 0 && ps < D;
                const __amdgpu_buffer_rsrc_t hsr = __builtin_amdgcn_make_buffer_rsrc(scur ? cx_cur.hsb : cx_prev.hsb, 0, 0x7FFFFF00, 0x00020000);
                const unsigned oh_ = scur ? cx_cur.ohs : cx_prev.ohs;
                const unsigned po = ok_ ? (unsigned)((long)ps * hs_planeB) : 0x80000000u;
                if constexpr (HP) {
                    // planar: one dword per (kh, kw) plane, 32 consecutive floats per lane half; half 1 has no fifth plane (dropped by its offset)
#pragma unroll
                    for (int j = 0; j < 5; ++j)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o_[j]), hsr, oh_ + (unsigned)j * hs_jB + (j == 4 && g ? 0x80000000u : po), 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b128(head_pack(o_), hsr, oh_ + (hs_drop0 ? 0x80000000u : po), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o_[4]), hsr, oh_ + 16 + (hs_drop1 ? 0x80000000u : po), 0, 0);
                }
            }
        };
        auto head_mfma = [&](int i) __attribute__((always_inline)) {
            if constexpr (HEAD) {
                if (i == 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { bh_[e] = vh[e]; bl_[e] = vl[e]; }
                    z_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1h, bh_, z_, 0, 0, 0);
                } else if (i == 1) {
                    z_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1h, bl_, z_, 0, 0, 0);
                } else {
                    z_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1l, bh_, z_, 0, 0, 0);
                    pkeep = z_;                  // (the previous P was consumed by head_update in groups 0..4)
                    if (k == 1) {
                        char* pb = pbuf + (gs & 1) * (2 * XW) + r * XW + lane * 16;
#pragma unroll
                        for (int q = 0; q < 4; ++q) *(f32x4*)(pb + q * 1024) = (f32x4){z_[q * 4], z_[q * 4 + 1], z_[q * 4 + 2], z_[q * 4 + 3]};
                    }
                }
            }
        };
        if constexpr (COMPUTE) {
            constexpr bool K0 = KIND != 2, K2 = KIND != 1;          // taps kd = 0 (plane t+1 exists), kd = 2 (plane t-1 exists)
            const __attribute__((address_space(3))) char* sb = ringl + J * SLAB + (FL ? cx_cur.bf : bfrag);
            f16x8 bh[2], bl[2];
            bh[0] = *(lds_frag*)(sb);
            bl[0] = *(lds_frag*)(sb + 4 * CPB);
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const int kh = q / 3, kw = q - kh * 3;
                if (q + 1 < 9) {
                    const int kh1 = (q + 1) / 3, kw1 = (q + 1) - kh1 * 3;
                    bh[(q + 1) & 1] = *(lds_frag*)(sb + (kh1 * SX + kw1) * 16);
                    bl[(q + 1) & 1] = *(lds_frag*)(sb + 4 * CPB + (kh1 * SX + kw1) * 16);
                }
                const f16x8 h_ = bh[q & 1], l_ = bl[q & 1];
                const int t0 = kh * 3 + kw, t1 = 9 + t0, t2 = 18 + t0;       // taps kd = 0, 1, 2
                if (q == OWN && !HEAD) stores();
                if (q < 8) {
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], h_, acc[A0], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], h_, acc[A1], 0, 0, 0);
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], h_, acc[A2], 0, 0, 0);
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], l_, acc[A0], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], l_, acc[A1], 0, 0, 0);
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], l_, acc[A2], 0, 0, 0);
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t0], h_, acc[A0], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t1], h_, acc[A1], 0, 0, 0);
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t2], h_, acc[A2], 0, 0, 0);
                    if (q < OWN) fin(q);
                    if (q < 5) head_update(q);
                    if (q == 5) head_store();
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    // last group: the finished plane's accumulator first, its publication in the shadow of the rest (HEAD: the three MFMAs of
                    // the cout-1 product in between: a dependent chain, each link behind independent work)
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], h_, acc[A2], 0, 0, 0);
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], h_, acc[A0], 0, 0, 0);
                    head_mfma(0);
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t2], l_, acc[A2], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], h_, acc[A1], 0, 0, 0);
                    if (K2) acc[A2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t2], h_, acc[A2], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    head_mfma(1);
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t0], l_, acc[A0], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[t1], l_, acc[A1], 0, 0, 0);
                    if (K0) acc[A0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t0], h_, acc[A0], 0, 0, 0);
                    acc[A1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[t1], h_, acc[A1], 0, 0, 0);
                    publish();
                    head_mfma(2);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < OWN; ++e) fin(e);
            if constexpr (HEAD) {
#pragma unroll
                for (int jj = 0; jj < 5; ++jj) head_update(jj);
                head_store();
                head_mfma(0); head_mfma(1); head_mfma(2);
            } else {
                stores();
            }
            publish();
        }
        ++gs;
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
#pragma unroll 1
    for (unsigned it = 0;; ++it) {
        const Col cnext = col_of(it + 1);
        s_next = cnext.valid ? src_of(cnext) : s_cur;
        step(0, I0{}, I1{});
        step(1, I1{}, I0{});
        if (Dw == 3) {
            step(2, I2{}, I2{});
        } else {
            step(2, I2{}, I0{});
#pragma unroll 1
            for (int t0 = 3; t0 + 3 < Dw; t0 += 3) {
                step(t0, I0{}, I0{});
                step(t0 + 1, I1{}, I0{});
                step(t0 + 2, I2{}, I0{});
            }
            step(Dw - 3, I0{}, I0{});
            step(Dw - 2, I1{}, I0{});
            step(Dw - 1, I2{}, I2{});
        }
        if (!cnext.valid) break;
        cx_prev = cx_cur;
        cx_cur = ctx_of(cnext);
        s_cur = s_next;
    }
    // drain: publish the last plane, finalize the last two
    step(Dw, I0{}, I3{});
    step(Dw + 1, I1{}, I3{});
    if constexpr (HEAD) {
        // the P of the last plane arrives a step after its finalize (it closes plane D - 2); then the column's last plane is complete
        step(Dw + 2, I2{}, I3{});
        const bool ok_ = k == 0 && cx_cur.ok;
        const __amdgpu_buffer_rsrc_t hsr = __builtin_amdgcn_make_buffer_rsrc(cx_cur.hsb, 0, 0x7FFFFF00, 0x00020000);
        const unsigned po = ok_ ? (unsigned)((long)(D - 1) * hs_planeB) : 0x80000000u;
        if constexpr (HP) {
#pragma unroll
            for (int j = 0; j < 5; ++j)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, SC[j]), hsr, cx_cur.ohs + (unsigned)j * hs_jB + (j == 4 && g ? 0x80000000u : po), 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b128(head_pack(SC), hsr, cx_cur.ohs + (hs_drop0 ? 0x80000000u : po), 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, SC[4]), hsr, cx_cur.ohs + 16 + (hs_drop1 ? 0x80000000u : po), 0, 0);
        }
    }
    og.flush(p.ovf);
}

// The flat head runs this body under a name of its own, convs16_headflat_kernel<2,false,0,28,false,false,true>: the row head
// stays the ONE fused-head instantiation of convs16_kernel that tests/test_isa_weights_in_agprs.py counts (tests/test_isa_head_flat.py holds
// the new kernel to the same caps).  A shared __device__ body behind two __global__ wrappers would do as well, but it changes the scalar
// register allocation of the other nineteen instantiations (tools/isa_step_stats.py: SGPR spills, lane moves); so the template above is
// compiled a second time, textually: this file includes itself once, and the second pass sees nothing but the template.
#ifndef CONVS16_SECOND_PASS
#define CONVS16_SECOND_PASS
#undef CONVS16_KERNEL
#define CONVS16_KERNEL convs16_headflat_kernel
#include "convs16.hip"
#undef CONVS16_KERNEL

constexpr long FLAT_MIN_COLUMNS = 2048;       // below: the row form (eight columns per workgroup; 256 Config-A ROIs have 3136)
constexpr long FLAT_HALF_GROUP = 8;           // the 64 -> 64 form on 14-column maps: units per group where the caller names none
constexpr long FLAT_HALF_MIN_COLUMNS = 1176;  // ... and its lower bound in columns of 32 voxels: 192 half-resolution Config-A ROIs, the smallest batch measured where a worker runs fewer columns (10 against 11)

// flat tiles: units per group -- dil bit 0x4000: 1; the 32 -> 32 form: else 4; the 64 -> 64 form: 0x8000: 8, 0x10000: 4, else FLAT_HALF_GROUP
inline long s16_flat_group(const drc_s16conv_params& p) {
    if (p.dil & 0x4000) return 1;
    if (p.cin != 64) return 4;
    return (p.dil & 0x8000) ? 8 : (p.dil & 0x10000) ? 4 : FLAT_HALF_GROUP;
}
// ... and the columns of a launch (64 voxels, 32 in the 64 -> 64 form; the last group may be short but is enumerated whole)
inline long s16_flat_columns(const drc_s16conv_params& p) {
    const long G = s16_flat_group(p), FV = p.cin == 64 ? 32 : 64;
    return (p.N + G - 1) / G * ((G * p.H * p.W + FV - 1) / FV);
}
// The 64 -> 64 form stages a column into the row form's chunk plane of 128 voxels = 8 stacked rows of 16, and counts units from the column's
// first one with three compares.  Whether every column of a launch stays inside both is decided here, by walking the columns of a whole group
// and of the short last one exactly as the kernel's col_of / src_of do (H = 1 | 2 can reach a fourth unit or a ninth row, depending on where
// the columns of a group of G units start).
inline bool s16_flat_half_fits(long N, long G, long H) {
    const long HW = H * 14, Hp1 = H + 1;
    const long tail = N % G;
    for (int pass = 0; pass < 2; ++pass) {
        const long gu = pass == 0 ? (N >= G ? G : 0) : tail;
        for (long f0 = 0; f0 < gu * HW; f0 += 32) {
            const long u0 = f0 / HW, rem0 = f0 - u0 * HW, y0 = rem0 / 14;
            const long lim = gu * HW - f0;
            const long el = rem0 + (lim < 32 ? lim : 32) - 1;
            const long du_l = el / HW;
            const long rr_last = du_l * Hp1 + (el - du_l * HW) / 14 - y0 + 2;
            if (du_l > 3 || rr_last > 7) return false;
        }
    }
    return true;
}

template <int KW, bool CV, int RT, int WT, bool RES, bool Y32, bool HEAD = false>
int launch2(const drc_s16conv_params& p, hipStream_t stream) {
    constexpr int CBI = KW / 2;
    constexpr bool FLAT = RT == 0;
    constexpr int SLAB = CBI * 8 * (FLAT && KW == 2 ? PV_FLAT : PV_ROWS) * 16;
    constexpr int XW = 4096;
    constexpr size_t lds = CV ? (size_t)s16cv::LDS_BYTES : RING * SLAB + 2 * 4 * XW + (HEAD ? 2 * 2 * XW : 0);
    static_assert(lds <= 160 * 1024, "LDS");
    static bool attr_done = false;
    void (*const kern)(const drc_s16conv_params) = [] {
        if constexpr (FLAT && HEAD) return convs16_headflat_kernel<KW, CV, RT, WT, RES, Y32, HEAD>;
        else return convs16_kernel<KW, CV, RT, WT, RES, Y32, HEAD>;
    }();
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    constexpr int rows = FLAT ? 1 : (4 / KW) * RT;
    const long columns = FLAT ? s16_flat_columns(p) : (long)p.N * ((p.H + rows - 1) / rows) * ((p.W + WT - 1) / WT);
    // one block per CU (the weights take the register file); a multiple of 8 so that every XCD runs the same number
    const int n_ct = p.cout / 32;
    long blocks = 256;                                   // column workers x cout tiles (the tiles of a worker side by side on its XCD)
    while (blocks > 8 * n_ct && blocks / (2 * n_ct) >= columns) blocks /= 2;
    if constexpr (CV) blocks = s16cv::s16_cvrows_blocks<1>(p);      // (its work items are rows, not columns of rows)
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, stream, p);
    return (int)hipGetLastError();
}

template <int KW, bool CV, int RT = 1, int WT = 28>
int launch(const drc_s16conv_params& p, hipStream_t stream) {
    if (p.head) {
        if constexpr (KW == 2 && !CV && RT == 1) return launch2<KW, CV, RT, WT, false, false, true>(p, stream);
        else return -4;
    }
    if (p.y32) {
        if constexpr (KW == 2 && !CV && RT == 1) return launch2<KW, CV, RT, WT, false, true>(p, stream);
        else return -4;
    }
    if constexpr (CV) return launch2<KW, CV, RT, WT, false, false>(p, stream);
    else return p.res ? launch2<KW, CV, RT, WT, true, false>(p, stream) : launch2<KW, CV, RT, WT, false, false>(p, stream);
}

}  // namespace

extern "C" int drc_conv3d_k3_s16_supported(int cin, int cout, int D, int H, int W) {
    if (cin != 32 && cin != 64) return 0;
    if (cout != 32 && cout != 64) return 0;
    // round 6: any D, H, W > 0 (the reference's contract is D, H, W = 0 mod 4 at this resolution, stackhourglass.py:115-128).  W <= 7: 4 x 7 tiles,
    // W <= 14: 2 x 14, else 1 x 28 -- the last x tile and the last row tile masked; D that is not a multiple of 3: the walk is padded with
    // phantom zero planes.  Full MFMA columns / no phantom work at W = 7 | 14 | 0 mod 28 and D = 0 mod 3 (the shapes of BASELINE's configs).
    return D > 0 && H > 0 && W > 0;
}

// The form a parameter block's launch takes (host code, no launch): 0 = row tiles; 1 | 4 | 8 = flat tiles in groups of that many units (the plain
// and the residual 32 -> 32 layer on 28-column maps, at least FLAT_MIN_COLUMNS columns; the 64 -> 64 layer on 14-column maps, at least
// FLAT_HALF_MIN_COLUMNS columns whose slabs all fit, s16_flat_half_fits; offsets of four units inside 32 bits); -4: flat tiles were asked for
// (dil bit 0x2000) where the form does not exist.  dil bit 0x1000 keeps the row form.
extern "C" int drc_conv3d_k3_s16_flat(const drc_s16conv_params* pp) {
    if (!pp) return -1;
    const drc_s16conv_params& p = *pp;
    const bool forced = p.dil & 0x2000;
    const long unit16 = (long)(p.D + 2) * (p.H + 2) * (p.W + 2) * 128;
    const bool half = p.cin == 64 && p.cout == 64 && p.W == 14;
    const bool shape = (p.cin == 32 && p.cout == 32 && p.W == 28) || half;
    // the fused head has the form where the caller asks for the planar layout of its partial sums (head_rows == DRC_HEAD_PLANAR: the only
    // layout a tile that is no image row can write); the head's depth rule (D >= 6, D % 3 == 0) and four units' planes inside 32 bits
    const bool hp = p.head && p.head_rows == DRC_HEAD_PLANAR;
    const bool out = hp ? !p.y16 && !p.res && !half && p.D >= 6 && p.D % 3 == 0 && 4L * p.D * p.H * p.W * 36 < 0x7FFFFF00L : p.y16 && !p.head;
    const bool can = shape && p.D > 0 && p.H > 0 && p.N > 0 && p.x && out && !p.y32 && !p.left && !p.right &&
                     4 * (p.cout / 32) * unit16 < 0x7FFFFF00L && (!half || s16_flat_half_fits(p.N, s16_flat_group(p), p.H));
    if (p.dil & 0x1000) return forced ? -1 : 0;
    if (!can) return forced ? -4 : 0;
    if (!forced && s16_flat_columns(p) < (half ? FLAT_HALF_MIN_COLUMNS : FLAT_MIN_COLUMNS)) return 0;
    return (int)s16_flat_group(p);
}

extern "C" int drc_conv3d_k3_s16_fwd(const drc_s16conv_params* pp, void* stream) {
    if (!pp) return -1;
    const drc_s16conv_params& p = *pp;
    const bool cv = p.left || p.right;
    if (!p.w || !p.scale || !p.shift) return -1;
    if (p.head) {                                                                   // fused cout-1 head: no tensor output, 32 -> 32 at full resolution
        if (!p.w1 || p.y16 || p.y32 || p.res || cv) return -1;
        if (p.cin != 32 || p.cout != 32 || p.W % 28 || p.D < 6 || p.D % 3) return -4;      // (the depth sums of the head close over real planes only)
        if (p.head_rows < 0 || p.head_rows > DRC_HEAD_PLANAR) return -1;
        if (p.head_rows && p.W != 28) return -4;                                    // the rows layout: one x tile per row; planar: the flat form's maps
        if ((long)p.D * p.H * p.W * 48 >= 0x7FFFFF00L) return -5;
    } else if (p.head_rows) return -1;
    else if (!p.y16 == !p.y32) return -1;                                         // exactly one output
    if (p.y32 && (p.res || p.cin != 32 || p.W <= 14)) return -4;                    // blocked fp32 output: the 32-channel layers on 1 x 28 tiles without residual
    if (cv && p.res) return -4;
    if (cv ? (!p.left || !p.right || p.cin != 64) : !p.x) return -1;
    if (p.N < 0) return -2;
    if (!drc_conv3d_k3_s16_supported(p.cin, p.cout, p.D, p.H, p.W)) return -4;
    if (cv && p.W <= 14) return -4;                                                 // the cost-volume form is built on 1 x 28 tiles
    if (p.N == 0) return 0;
    // 32-bit offsets inside one unit
    const long unit16 = (long)(p.cout / 32) * (p.D + 2) * (p.H + 2) * (p.W + 2) * 128;
    if (unit16 >= 0x7FFFFF00L / 2) return -5;
    hipStream_t s = (hipStream_t)stream;
    if (drc_conv3d_k3_s16_wide(pp)) return drc_conv3d_k3_s16_wide_fwd(pp, stream);      // the cost-volume form at large batches: two tiles per wave (convs16w.hip)
    if (cv) return launch<4, true>(p, s);
    int flat = drc_conv3d_k3_s16_flat(pp);
    if (p.head && p.head_rows == DRC_HEAD_PLANAR && flat == 0) {
        // the layout is the caller's word: a planar head IS the flat form, whatever the launch's size (the caller asks drc_conv3d_k3_s16_flat
        // first where it wants the library's choice); no such form for this block: -4
        drc_s16conv_params f = p;
        f.dil = (p.dil & ~0x1000) | 0x2000;
        flat = drc_conv3d_k3_s16_flat(&f);
    }
    if (flat < 0) return flat;
    if (flat) {
        drc_s16conv_params q = p;                   // the kernel reads the group size from the bits alone
        q.dil = (p.dil & ~0x1C000) | (flat == 1 ? 0x4000 : flat == 8 ? 0x8000 : 0x10000);
        if (p.head) return launch2<2, false, 0, 28, false, false, true>(q, s);
        if (p.cin == 64) return p.res ? launch2<4, false, 0, 14, true, false>(q, s) : launch2<4, false, 0, 14, false, false>(q, s);
        return p.res ? launch2<2, false, 0, 28, true, false>(q, s) : launch2<2, false, 0, 28, false, false>(q, s);
    }
    if (p.W <= 7) return p.cin == 32 ? launch<2, false, 4, 7>(p, s) : launch<4, false, 4, 7>(p, s);
    if (p.W <= 14) return p.cin == 32 ? launch<2, false, 2, 14>(p, s) : launch<4, false, 2, 14>(p, s);
    return p.cin == 32 ? launch<2, false>(p, s) : launch<4, false>(p, s);
}
#endif  // CONVS16_SECOND_PASS
