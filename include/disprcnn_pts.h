/*
 * disprcnn_pts.h -- C ABI of libdisprcnn_pts.so (MI355X / gfx950 only): the 3D stage's point ops.
 *
 * Kept apart from libdisprcnn_hip.so so that the regressor's source digest (csrc/build.py:source_digest) does not move.
 * Same conventions as disprcnn_hip.h:
 *   - the CALLER allocates every buffer; the library never allocates, frees or syncs;
 *   - all pointers are device pointers, fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void*;
 *   - return 0 on success, <0 for a bad argument / unsupported shape, >0 = hipError_t after the launch.
 */
#ifndef DISPRCNN_PTS_H
#define DISPRCNN_PTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* "disprcnn_pts gfx950 <abi-version>" */
const char* drc_pts_version(void);

/* ---------------------------------------------------------------------------------------
 * Instance point clouds: PointRCNN.process_input_eval + back_project (point_rcnn.py:37-83, 189-241), eval form.
 *
 * Per ROI r (all images in one launch):
 *   roi_i [R,8] int32 : x1, y1, x2, y2, x1p, x2p (expand_box_to_integer of the left / right boxes), image H, image W
 *   roi_f [R,12] fp32 : left box x1, y1, x2, y2 (float, for the Masker paste and the rotation), fu, fv, cu, cv, tx, ty,
 *                       stereo_fuxbaseline, half width of the FIRST image (rotate_pc_along_y)
 *   roi_d [R]  fp64   : fu (the rotation angle is atan2 in double, as the reference's float64 `fus` tensor makes it)
 *   disp  [R,S,S]     : per-ROI disparity;   mask [R,M,M]: mask probabilities (Masker padding `pad`, threshold `thresh`)
 *
 * drc_instance_points_fwd (kernel A): one workgroup per ROI compacts, in x-major order (meshgrid(x, y)), the flat image
 * index y*W + x of every box pixel whose masked depth is > 0 into ws[off_r ...]; off_r = sum of the clipped box areas of
 * the ROIs before r.  info [2R+1] int64: info[r] = count_r, info[R + r] = off_r, info[2R] = total area.  Nothing is written
 * to ws when the total area exceeds `ws_cap` (the counts are still right): the caller grows ws and launches again.
 *
 * drc_instance_points_gather_fwd (kernel B): pts[r,i] = point of ws[off_r + choice[r,i]] (choice [R,npoints] int32 < count_r),
 * z clamped to max_depth, rotated about y by rot[r] = atan2(box centre x - half_w0, fu), minus the per-ROI mean (a fixed-order
 * sum: bit-identical run to run).  pts [R,npoints,3], mean [R,3], rot [R] fp64, src_pix [R,npoints] int32 (nullable).
 * ------------------------------------------------------------------------------------- */
int drc_instance_points_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const float* mask, int M, int pad,
                            float thresh, int R, int64_t* info, int32_t* ws, int64_t ws_cap, void* stream);
int drc_instance_points_gather_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const double* roi_d, int R,
                                   const int64_t* info, const int32_t* ws, const int32_t* choice, int npoints, float max_depth,
                                   float* pts, float* mean, double* rot, int32_t* src_pix, void* stream);

/* The training forms (PointRCNN.process_input + back_project with fix_seed=False): the same two kernels, same arguments and layouts.
 * drc_instance_points_train_fwd: depth = fuxb / (disp + 1e-6) without the lower clamp at 1, so a pixel of negative depth is dropped by
 * the z > 0 filter; the mask is applied when a masked box pixel has positive depth.
 * drc_instance_points_gather_train_fwd: after the clamp at max_depth the point is multiplied by `scale`, x is negated when `flip`, and
 * the rotation angle is negated when `flip`; rot[r] is the signed angle that was used. */
int drc_instance_points_train_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const float* mask, int M, int pad,
                                  float thresh, int R, int64_t* info, int32_t* ws, int64_t ws_cap, void* stream);
int drc_instance_points_gather_train_fwd(const float* disp, int S, const int32_t* roi_i, const float* roi_f, const double* roi_d, int R,
                                         const int64_t* info, const int32_t* ws, const int32_t* choice, int npoints, float max_depth,
                                         float scale, int flip, float* pts, float* mean, double* rot, int32_t* src_pix, void* stream);

/* drc_match_targets_fwd: PointRCNN.match_targets_to_proposals for all images in one launch.  boxes [R,4] left proposals (xyxy), span
 * [R,2] int32 = (first, count) of the ground truths of the proposal's image in gt [G,4] (xyxy) and gt_rows [G,row] (the targets' 3D
 * boxes).  IoU with TO_REMOVE = 1 in fp32 as boxlist_iou, the max over the ground truths (ties to the lowest index), then
 * Matcher(high, low, allow_low_quality_matches=False): matched [R] int64 = the index within the image, -1 below `low`, -2 below `high`;
 * out_rows [R,row] = gt_rows at the index clamped at 0 (zeros when the image has no ground truth, where matched is -1). */
int drc_match_targets_fwd(int R, int G, const float* boxes, const int32_t* span, const float* gt, const float* gt_rows, int row,
                          float high, float low, int64_t* matched, float* out_rows, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointNet++ operator set (pointnet2_lib/pointnet2/src/pointnet2_api.cpp).  Layouts as the reference's *_gpu.cu.
 * ------------------------------------------------------------------------------------- */
/* xyz [B,N,3] -> idx [B,M]; temp [B,N] (pre-filled 1e10 by the caller) receives the final min-distances.
 * block_size = opt_n_threads(N) of the reference (cuda_utils.h): ties resolve as its tree reduction does.  N <= 16384. */
int drc_pn2_furthest_point_sampling(int B, int N, int M, const float* xyz, float* temp, int32_t* idx, int block_size, void* stream);
/* points [B,C,N], idx [B,M] -> out [B,C,M] */
int drc_pn2_gather_points(int B, int C, int N, int M, const float* points, const int32_t* idx, float* out, void* stream);
/* new_xyz [B,M,3], xyz [B,N,3] -> idx [B,M,nsample] (rows without a hit are left as the caller initialised them) */
int drc_pn2_ball_query(int B, int N, int M, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx, void* stream);
/* points [B,C,N], idx [B,M,nsample] -> out [B,C,M,nsample] */
int drc_pn2_group_points(int B, int C, int N, int M, int nsample, const float* points, const int32_t* idx, float* out, void* stream);
/* unknown [B,N,3], known [B,M,3] -> dist2 [B,N,3], idx [B,N,3] */
int drc_pn2_three_nn(int B, int N, int M, const float* unknown, const float* known, float* dist2, int32_t* idx, void* stream);
/* points [B,C,M], idx/weight [B,N,3] -> out [B,C,N] */
int drc_pn2_three_interpolate(int B, int C, int M, int N, const float* points, const int32_t* idx, const float* weight, float* out,
                              void* stream);

/* Deterministic scatter-add backward through a per-source CSR of an index tensor.
 * sorted_keys [B,E]: each batch row of the index tensor sorted stably (entry order kept among equal keys) -> seg_start/seg_end
 * [B,N] (zeroed by the caller): the run of each source n.  Keys outside [0,N) are skipped.
 * grad_src[b,c,n] += sum over the run of n, in entry order, of grad_out[b,c,perm[b,j] / per_col] (* weight[b,perm[b,j]]).
 * gather: per_col 1, K = M; group: per_col 1, K = M*nsample; three_interpolate: per_col 3, K = N (weight [B,N*3]). */
int drc_pn2_csr_bounds(int B, int E, int N, const int32_t* sorted_keys, int32_t* seg_start, int32_t* seg_end, void* stream);
int drc_pn2_csr_scatter_add(int B, int C, int N, int K, int E, int per_col, const float* grad_out, const int32_t* perm,
                            const int32_t* seg_start, const int32_t* seg_end, const float* weight, float* grad_src, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointRCNN 3D box ops (point_rcnn/lib/utils/iou3d/src/iou3d_kernel.cu, roipool3d/src/roipool3d_kernel.cu).  fp32, evaluated in
 * the reference's expression order.
 * ------------------------------------------------------------------------------------- */
/* a [Na,5], b [Nb,5] as [x1,y1,x2,y2,ry] -> out [Na,Nb]: mode 0 = rotated BEV overlap area (box_overlap), 1 = BEV IoU (iou_bev) */
int drc_box3d_bev(int Na, int Nb, const float* a, const float* b, int mode, float* out, void* stream);
/* a [Na,7], b [Nb,7] as [x,y,z,h,w,l,ry] -> out [Na,Nb]: boxes_iou3d_gpu (BEV conversion, overlap, height overlap, volumes, the
 * clamp(min=1e-7) division) in one kernel */
int drc_box3d_iou3d(int Na, int Nb, const float* a, const float* b, float* out, void* stream);
/* Batched greedy NMS (nms_gpu / nms_normal_gpu of iou3d.cpp) of B rows at once.  boxes [B,Nmax,5], each row already in score
 * order; counts [B] int32 (clamped to [0,Nmax]).  normal != 0: axis-aligned iou_normal, else rotated iou_bev; a box is suppressed
 * when its IoU with a kept one is > thresh.  mask: B * Nmax * ceil(Nmax/64) words of workspace (contents need not be set).
 * keep [B,keep_stride] int64 <- kept positions in row order, num_keep [B] int32 <- their count; a row stops after max_keep kept
 * (max_keep <= 0: no limit), keep_stride >= min(max_keep, Nmax).  Nmax <= 32768.  Entries past num_keep are left untouched. */
int drc_box3d_nms(int B, int Nmax, const float* boxes, const int32_t* counts, float thresh, int normal, int max_keep, uint64_t* mask,
                  int64_t* keep, int keep_stride, int32_t* num_keep, void* stream);
/* roipool3dLauncher: xyz [B,N,3], boxes3d [B,M,7] (already enlarged), feat [B,N,C] -> pooled [B,M,S,3+C] (xyz ++ feature of the
 * first S in-box points in index order, repeated cyclically when fewer), empty_flag [B,M] int32 <- 1 for a box with no point (its
 * rows and the other flags are left as the caller zeroed them).  In-box test: pt_in_box3d, max_dis 10.  S <= drc_box3d_max_pool_samples(). */
int drc_roipool3d_fwd(int B, int N, int M, int C, int S, const float* xyz, const float* boxes3d, const float* feat, float* pooled,
                      int32_t* empty_flag, void* stream);
int drc_box3d_max_pool_samples(void);
/* xyz [B,N,3], boxes3d [B,M,7] -> flags [B,M,N] uint8 (0/1): pt_in_box3d of every point and box */
int drc_pts_in_boxes3d(int B, int N, int M, const float* xyz, const float* boxes3d, uint8_t* flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointRCNN RPN: shared MLPs on fp32 MFMA (v_mfma_f32_32x32x2_f32, fp32 accumulate) and the proposal decode (pts/pn2_mlp.hip).
 *
 * Weights are BatchNorm-folded by the caller and passed K-MAJOR: wt_l [Cin_l, Cout_l] (the transpose of the conv weight
 * W_l [Cout_l, Cin_l]), bias b_l [Cout_l].  Outputs go into a [B, c_total, *] buffer at channel offset c_off.
 * ------------------------------------------------------------------------------------- */
/* Fused group -> shared MLP (ReLU after every layer) -> max over the neighbourhood:
 *   out[b, c_off + c, m] = max_s MLP(concat(xyz[b, idx[b,m,s]] - new_xyz[b,m], feats[b, :, idx[b,m,s]]))[c]
 * xyz [B,N,3], new_xyz [B,M,3], feats [B,C,N] (null when C = 0), idx [B,M,nsample] int32 (values are clamped to [0,N)).
 * n_layers in 1..3 (unused layers: null, 0); Cin_0 = C + 3, Cin_l = Cout_{l-1}.  1 <= nsample <= 64; any C >= 0 and Cout >= 1 for the
 * last layer; a hidden layer's width is bounded by the LDS image that holds it (512).  -3: widths not supported. */
int drc_pn2_sa_mlp_max_fwd(int B, int N, int M, int C, int nsample, const float* xyz, const float* new_xyz, const float* feats,
                           const int32_t* idx, int n_layers, const float* wt0, const float* b0, int cout0, const float* wt1, const float* b1,
                           int cout1, const float* wt2, const float* b2, int cout2, float* out, int c_total, int c_off, void* stream);
/* out[b, c_off + c, n] = act(sum_k wt[k, c] * concat(in0 [B,C0,N], in1 [B,C1,N])[b, k, n] + bias[c]); in1 null when C1 = 0;
 * relu != 0: ReLU, else no activation. */
int drc_pn2_pointwise_mlp_fwd(int B, int N, int C0, int C1, const float* in0, const float* in1, const float* wt, const float* bias, int cout,
                              int relu, float* out, int c_total, int c_off, void* stream);
/* decode_bbox_target in the RPN's form (get_y_by_bin = False, get_ry_fine = False; first-maximum argmax), then y += h / 2, and
 * boxes3d_to_bev in the same pass: xyz [n,3], reg [n,R] -> boxes [n,7] (x, y, z, h, w, l, ry), bev [n,5] (x1, y1, x2, y2, ry).
 * R = per_loc_bin_num * (xz_fine ? 4 : 2) + 1 + 2 * num_head_bin + 3.  The constants are the reference's Python doubles rounded to
 * fp32 by the caller: half_bin = loc_bin_size / 2, angle_per_class = 2 pi / num_head_bin, half_angle = angle_per_class / 2.
 * fp32 in the reference's expression order (the library is built without FP contraction); the wrap is torch's remainder. */
int drc_rpn_decode_proposals(int64_t n, int R, const float* xyz, const float* reg, int per_loc_bin_num, int num_head_bin, int xz_fine,
                             float loc_bin_size, float half_bin, float loc_scope, float angle_per_class, float half_angle, float two_pi,
                             float pi, float anchor_h, float anchor_w, float anchor_l, float* boxes, float* bev, void* stream);
/* xyz [n,3] -> out [n] = |p| (RPN's pts_depth): sqrt(fma(z, z, fma(y, y, x * x))), the rounding of torch's CPU norm reduction, which
 * the reference's recordings were made with; bit-identical on every device. */
int drc_rpn_points_depth(int64_t n, const float* xyz, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Backward of the shared MLPs (pts/pn2_mlp_bwd.hip): one pointwise layer out = act(W . concat(in0, in1) + b) with the conv weight in its
 * OWN layout W [Cout, Cin] (Cin = C0 + C1), and the max over a neighbourhood with its winner.  fp32, [B, C, N] channel-major.  With
 * gZ = gout (.) [out > 0] when relu != 0 (out: the layer's output, may be null otherwise), gZ = gout when relu == 0; the mask is applied
 * while the operand is loaded.  No atomics, no allocation, no synchronisation; -1 bad arguments, -2 limits (B <= 65535).
 * ------------------------------------------------------------------------------------- */
/* gin [B, C0 + C1, N] <- W^T . gZ on fp32 MFMA; the two inputs' gradients are its channel ranges.  Every element is written. */
int drc_pn2_pointwise_mlp_dgrad(int B, int N, int C0, int C1, int cout, int relu, const float* gout, const float* out, const float* w,
                                float* gin, void* stream);
/* The number of columns of the flattened (b, n) axis one partial sum covers. */
int drc_pn2_wgrad_chunk(void);
/* Floats of workspace drc_pn2_pointwise_mlp_wgrad needs: ceil(B N / chunk) * Cout * (Cin + 1); -1 for bad arguments. */
int64_t drc_pn2_wgrad_workspace_floats(int B, int N, int C0, int C1, int cout);
/* gw [Cout, Cin] <- sum_{b,n} gZ[b, co, n] X[b, ci, n], gb [Cout] <- sum_{b,n} gZ[b, co, n] (either may be null, not both).  Split over the
 * columns: fp32 MFMA partials per chunk into `workspace` (contents need not be set), then added in fp64 in chunk order and rounded once:
 * the same bits run to run, which depend on the chunk length. */
int drc_pn2_pointwise_mlp_wgrad(int B, int N, int C0, int C1, int cout, int relu, const float* gout, const float* out, const float* in0,
                                const float* in1, float* workspace, float* gw, float* gb, void* stream);
/* x [rows, ns] (rows = B C M) -> out [rows] = max over ns, arg [rows] int32 (may be null) = the winner's sample, ties to the lowest index.
 * 1 <= ns <= 64. */
int drc_pn2_group_max_fwd(int64_t rows, int ns, const float* x, float* out, int32_t* arg, void* stream);
/* gin [rows, ns] <- gout [rows] at arg [rows], zero elsewhere; every element is written. */
int drc_pn2_group_max_bwd(int64_t rows, int ns, const float* gout, const int32_t* arg, float* gin, void* stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm with batch statistics for the shared MLPs (pts/pn2_bn.hip): torch.nn.BatchNorm1d / 2d in training mode over an fp32
 * activation [B, C, N], channel-major (N = M * nsample for an SA level: every grouped column counts, padded duplicates included).
 * The statistic of channel c runs over its n = B * N values.  Every sum is fp64 in a fixed order: a grid of (column chunk, channel)
 * workgroups writes partials into a caller-provided fp64 workspace and a second launch adds them in chunk order.  No atomics: the same
 * bits run to run, which depend on the chunk length.  16-byte loads and stores when N % 4 == 0 and every tensor base is 16-byte aligned,
 * scalar ones otherwise.  No allocation, no copy, no synchronisation; -1 bad arguments (n < 2, C < 1, B < 1, N < 1, a null pointer),
 * -2 limits (C <= 65535).
 * ------------------------------------------------------------------------------------- */
/* The number of columns of the flattened (b, n) axis one partial sum covers. */
int drc_pn2_bn_chunk(void);
/* Doubles of workspace the two reducing entry points need: 2 * C * (ceil(B N / chunk) + 1); -1 for bad arguments. */
int64_t drc_pn2_bn_workspace_doubles(int B, int C, int N);
/* mean_invstd [2, C] <- the mean of y over (b, n) and 1 / sqrt(var + eps), var the biased variance, each rounded once from fp64.
 * running_mean, running_var [C] (both null, or both given) are updated in place as torch does:
 * r <- (1 - momentum) r + momentum * (mean | var * n / (n - 1)).  `workspace` need not be set. */
int drc_pn2_bn_stats(int B, int C, int N, const float* y, double* workspace, float eps, float momentum, float* mean_invstd,
                     float* running_mean, float* running_var, void* stream);
/* z <- act(gamma (y - mean) invstd + beta), act = ReLU when relu != 0, else the identity; one pass, every element is written. */
int drc_pn2_bn_apply_fwd(int B, int C, int N, int relu, const float* y, const float* mean_invstd, const float* gamma, const float* beta,
                         float* z, void* stream);
/* With g = gz (.) [z > 0] when relu != 0 (z may be null otherwise), xh = (y - mean) invstd, s1 = sum g, s2 = sum g xh over (b, n):
 * gy <- gamma invstd (g - s1 / n - xh s2 / n), ggamma [C] <- s2, gbeta [C] <- s1 (each rounded once from fp64).  Two passes over the
 * columns with the fixed-order sum of the partials between them.  Every element of gy is written. */
int drc_pn2_bn_bwd(int B, int C, int N, int relu, const float* gz, const float* z, const float* y, const float* mean_invstd,
                   const float* gamma, double* workspace, float* gy, float* ggamma, float* gbeta, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointRCNN RCNN stage (pts/rcnn_ops.hip; rcnn_net.py's ROI_SAMPLE_JIT eval branch, rcnn_inference.py).
 * ------------------------------------------------------------------------------------- */
/* ROI pooling fused with the canonical transform, one workgroup per (cloud, ROI), in the layouts the RPN returns and the shared MLPs
 * read: rpn_xyz [B,N,3], feat [B,C,N] (channel-major; null when C = 0), seg_mask [B,N], pts_depth [B,N] (read when use_depth != 0),
 * rois [B,M,7] as [x,y,z,h,w,l,ry] (NOT enlarged: the kernel applies enlarge_box3d with extra_width and extra_width2 = the caller's
 * fp32 rounding of 2 * extra_width).  For r = b * M + m and E = 1 + (use_depth != 0):
 *   xyz  [R,S,3]    <- (p - roi centre) rotated about y by roi ry, p = the first S in-box points in index order, repeated cyclically
 *   pts  [R,3+E,S]  <- canonical x, y, z, seg_mask, pts_depth / 70 - 0.5
 *   ofeat [R,C,S]   <- feat[b, :, selected]
 *   empty_flag [R] int32 <- 1 for a ROI without a point: its features are 0 (the depth channel too) and its xyz is rotate(0 - centre).
 * Every element of every output is written.  In-box test: pt_in_box3d, max_dis 10.  1 <= S <= drc_box3d_max_pool_samples(). */
int drc_rcnn_pool_canonical_fwd(int B, int N, int M, int C, int S, const float* rpn_xyz, const float* feat, const float* seg_mask,
                                const float* pts_depth, int use_depth, const float* rois, float extra_width, float extra_width2, float* xyz,
                                float* pts, float* ofeat, int32_t* empty_flag, void* stream);
/* decode_bbox_target in the RCNN's form (get_xz_fine = True, get_ry_fine = True, get_y_by_bin = y_by_bin; first-maximum argmax): the
 * rotation by -roi_ry, ry + roi_ry, the ROI's centre added on x and z (y = roi_y + offset), then boxes3d_to_bev and the sigmoid of the
 * class logit in the same pass: rois [n,7], reg [n,R], cls [n] -> boxes [n,7], bev [n,5], norm_score [n].
 * R = 4 * per_loc_bin_num + (y_by_bin ? 2 * loc_y_bin_num : 1) + 2 * num_head_bin + 3.  Constants as drc_rpn_decode_proposals: the
 * reference's Python doubles rounded to fp32 by the caller (half_bin = loc_bin_size / 2, half_y_bin = loc_y_bin_size / 2,
 * angle_per_class = (pi / 2) / num_head_bin, half_angle = angle_per_class / 2, quarter_pi = pi / 4). */
int drc_rcnn_decode_boxes(int64_t n, int R, const float* rois, const float* reg, const float* cls, int per_loc_bin_num, int loc_y_bin_num,
                          int num_head_bin, int y_by_bin, float loc_bin_size, float half_bin, float loc_scope, float loc_y_bin_size,
                          float half_y_bin, float loc_y_scope, float angle_per_class, float half_angle, float quarter_pi, float anchor_h,
                          float anchor_w, float anchor_l, float* boxes, float* bev, float* norm_score, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointRCNN's ProposalTargetLayer (pts/proposal_target.hip; rpn/proposal_target_layer.py): the RCNN stage's training ROIs.  Neither
 * entry synchronises or reads anything back.  Every random decision reads one fp32 uniform in [0,1) of `draws` [B, draw_stride]; per
 * cloud, with M candidates, P slots and T = ROI_FG_AUG_TIMES:  key[M] | pick[P] | noise[P][T][9] | aug[P][3]
 *   key:   the k foreground candidates with the smallest keys are taken, in key order (ties to the lower index): randperm(fg)[:k]
 *   pick:  slot j takes candidate min(floor(pick[j] * n), n - 1) of its class, in index order
 *   noise: per iteration [0] keep (kept when (double)u < 0.2), [1] range row min(floor(u * 5), 4), [2:5] position, [5:8] h w l, [8] angle
 *   aug:   rotation, scale, flip of data_augmentation
 * ------------------------------------------------------------------------------------- */
int drc_rcnn_sample_max_candidates(void); /* 1024: LDS lists */
int drc_rcnn_sample_max_slots(void);      /* 256: one lane per slot, one workgroup per cloud */
/* sample_rois_for_rcnn, one workgroup per cloud: cand [B,M,7], gt [B,N,7] as [x,y,z,h,w,l,ry] -> rois [B,P,7] (after the noise loop),
 * gt_of_rois [B,P,7], roi_iou [B,P], src_index [B,P] int32 (the candidate of each slot), n_iter [B,P] int32 (noise iterations run),
 * counts [B,5] int32: fg, hard bg, easy bg candidates, fg slots, and 1 for a cloud with no fg and no bg candidate (its slots take
 * candidates j mod M without noise; the reference raises there).  Slots: fg, hard bg, easy bg.  fg: iou >= fg_thresh
 * (= min(REG_FG_THRESH, CLS_FG_THRESH), also the loop's stop); hard: bg_thresh_lo <= iou < bg_thresh; easy: iou < bg_thresh_lo;
 * hard slots = (int)(bg slots * hard_bg_ratio) in double when both exist.  method 0: REG_AUG_METHOD 'multiple', 1: 'single'.
 * 1 <= M <= drc_rcnn_sample_max_candidates(), 1 <= P <= drc_rcnn_sample_max_slots(), N >= 1, T >= 0, 0 <= fg_per_image <= P,
 * draw_stride >= M + P + 9 P T + 3 P; otherwise -2 before any launch. */
int drc_rcnn_sample_rois(int B, int M, int N, int P, int T, int fg_per_image, int method, float fg_thresh, float bg_thresh,
                         float bg_thresh_lo, double hard_bg_ratio, const float* cand, const float* gt, const float* draws,
                         int64_t draw_stride, float* rois, float* gt_of_rois, float* roi_iou, int32_t* src_index, int32_t* n_iter,
                         int32_t* counts, void* stream);
/* The training form of drc_rcnn_pool_canonical_fwd, one workgroup per (cloud, slot); inputs as there plus the sampler's rois, gt_of_rois,
 * roi_iou [B,P(,7)] and counts [B,5].  The first S points inside the enlarged ROI are pooled; with aug != 0 the slot's rotation
 * ((u - 1) * rot_range, rot_range = pi / AUG_ROT_RANGE), scale (1 + ((u - 0.5) / 0.5) * 0.05) and flip (sign(u - 0.5); 0 is no flip) from
 * aug_draws [B, draw_stride] (the aug block: 3 per slot) are applied to the pooled coordinates, the ROI and its ground truth; then the
 * canonical transform.  With aug == 0 no draw is read.  For r = b * P + slot:
 *   xyz [R,S,3], pts [R,3+E,S], ofeat [R,C,S], empty_flag [R] int32 as drc_rcnn_pool_canonical_fwd (mask, depth, features un-augmented)
 *   roi_boxes3d [R,7]  the augmented ROI;  gt_ct [R,7]  its ground truth: centre - ROI centre, ry - (roi_ry mod 2 pi), rotated by that
 *   reg_valid_mask [R] int64 = iou > reg_fg & non-empty;  cls_label [R] int64 = iou > cls_fg, or -1 when empty or cls_bg < iou < cls_fg
 *   a cloud flagged in counts[b][4]: cls_label -1, reg_valid_mask 0.
 * Every element of every output is written.  1 <= S <= drc_box3d_max_pool_samples(). */
int drc_rcnn_pool_target_fwd(int B, int N, int P, int C, int S, const float* rpn_xyz, const float* feat, const float* seg_mask,
                             const float* pts_depth, int use_depth, const float* rois, const float* gt_of_rois, const float* roi_iou,
                             const int32_t* counts, const float* aug_draws, int64_t draw_stride, int aug, float rot_range, float extra_width,
                             float extra_width2, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh, float* xyz, float* pts,
                             float* ofeat, int32_t* empty_flag, float* roi_boxes3d, float* gt_ct, int64_t* cls_label,
                             int64_t* reg_valid_mask, void* stream);

/* ---------------------------------------------------------------------------------------
 * PointRCNN training labels and losses (pts/train_targets.hip; net/point_rcnn.py:generate_rpn_training_labels, utils/loss_utils.py,
 * net/rpn_loss.py, net/rcnn_loss.py).  Labels are the reference's fp32 expressions in its order; loss values are evaluated and summed in
 * fp64 (per-block partials added in block order, no atomics: bit-identical run to run) and rounded once.  No entry synchronises.
 * `scratch`: drc_train_scratch_doubles() doubles of workspace, contents need not be set.
 * ------------------------------------------------------------------------------------- */
int drc_train_scratch_doubles(void);
/* pts [B,N,3], one ground-truth box per cloud: boxes [B,7] as [x,y,z,h,w,l,ry], its corners [B,8,3] and the corners of the box enlarged
 * by 0.2 [B,8,3] -> cls_label [B,N] (1 inside, -1 where the two inside tests differ, else 0), reg_label [B,N,7] (centre - p with
 * centre.y = y - h / 2, then h, w, l, ry; zero on points that are not inside).  Inside (filter_bbox_3d): 0 < m < v.v, strictly, for the
 * dot products m of p - c4 with the edges v = c5 - c4, c0 - c4, c7 - c4.  Every element is written.  B <= 65535. */
int drc_rpn_point_labels(int B, int N, const float* pts, const float* boxes, const float* corners, const float* corners_large,
                         float* cls_label, float* reg_label, void* stream);
/* get_reg_loss.  pred_reg [rows,C], reg_label [rows,7] as [dx,dy,dz,h,w,l,ry], row_mask [rows] uint8 (the rows that take part: the
 * reference's `[fg_mask]` selection), loss_mask [rows] uint8 or null, anchor [3] or [rows,3].
 * opt and cst are HOST arrays.  opt [8] int32: per_loc_bin_num, loc_y_bin_num, num_head_bin, get_xz_fine, get_y_by_bin, get_ry_fine, anchor
 * per row, 0.  cst [17] fp32, the reference's Python doubles rounded by the caller: loc_scope, 2 loc_scope - 1e-3, loc_bin_size,
 * loc_bin_size / 2, the same four for y, angle_per_class, angle_per_class / 2, 2 pi, pi, pi * 0.5, pi * 1.5, pi * 0.25, 1e-3, pi * 0.5 - 1e-3.
 * C = per_loc_bin_num * (xz_fine ? 4 : 2) + (y_by_bin ? 2 * loc_y_bin_num : 1) + 2 * num_head_bin + 3 <= 128, every bin count <= 64; else -3.
 *
 * drc_bin_reg_targets: bins [rows,4] int32 <- x, z, y (-1 when y is not binned), ry bin labels; res [rows,7] <- the normalised residual
 *   labels x, z, y (the y offset itself when not binned), ry, and the three size residuals.  The code path of the loss.
 * drc_bin_reg_loss_fwd: sums [16] fp64 (kept for the backward) and terms [16] fp32 <- 0 x_bin, 1 z_bin, 2 x_res, 3 z_res, 4 y_offset or
 *   y_bin, 5 y_res, 6 ry_bin, 7 ry_res, 8 size, 9 loss_loc, 10 loss_angle, 11 loss_size, 12 selected rows, 13 selected rows with loss_mask.
 *   With a loss_mask every term is sum / mask count (the size term too: not divided by 3), without one the mean (size over 3 rows); the
 *   binned y terms are plain means in both cases; a zero count divides by nothing.
 * drc_bin_reg_loss_bwd: grad_pred [rows,C] <- d (g_loc loss_loc + g_angle loss_angle + g_size loss_size) / d pred_reg, zero on unselected
 *   rows; g_* are device scalars (null: 0).  Every element is written. */
int drc_bin_reg_targets(int64_t rows, int C, const float* reg_label, const float* anchor, const int32_t* opt, const float* cst,
                        int32_t* bins, float* res, void* stream);
int drc_bin_reg_loss_fwd(int64_t rows, int C, const float* pred_reg, const float* reg_label, const uint8_t* row_mask,
                         const uint8_t* loss_mask, const float* anchor, const int32_t* opt, const float* cst, double* sums, float* terms,
                         double* scratch, void* stream);
int drc_bin_reg_loss_bwd(int64_t rows, int C, const float* pred_reg, const float* reg_label, const uint8_t* row_mask,
                         const uint8_t* loss_mask, const float* anchor, const int32_t* opt, const float* cst, const double* sums,
                         const float* g_loc, const float* g_angle, const float* g_size, float* grad_pred, void* stream);
/* The point classification losses over logits [n], labels [n] fp32 (1 foreground, 0 background, -1 ignored), mask [n] uint8 or null.
 *   kind 1 BinaryCrossEntropy: weight fg_weight on foreground, sum over (label >= 0 and mask) / clamp(their count, 1); in the stable
 *          form max(x,0) - x t + log1p(exp(-|x|)), gradient w (sigmoid(x) - t) / count (no clamp of log(1 - p) at 100)
 *   kind 2 SigmoidFocalLoss (alpha, gamma): weights (pos + neg) / clamp(pos count, 1) over the masked rows
 *   kind 3 DiceLoss: 1 - sum min(p, t) / clamp(sum max(p, t), 1) over label != ignore_target (pass mask = null: the reference has none)
 * sums [16] fp64 (kept for the backward), terms [8] fp32 <- 0 loss, 1 / 2 its positive and negative parts (focal), 3 the normaliser before
 * the clamp.  bwd: grad_logits [n] <- grad_out[0] * d loss / d logits, every element written. */
int drc_point_cls_loss_fwd(int64_t n, int kind, const float* logits, const float* labels, const uint8_t* mask, float fg_weight, float alpha,
                           float gamma, float ignore_target, double* sums, float* terms, double* scratch, void* stream);
int drc_point_cls_loss_bwd(int64_t n, int kind, const float* logits, const float* labels, const uint8_t* mask, float fg_weight, float alpha,
                           float gamma, float ignore_target, const double* sums, const float* grad_out, float* grad_logits, void* stream);

/* SigmoidFocalClassificationLoss.forward, unreduced, over n elements: with grad_out null, out[i] <- (1 - p_t)^gamma alpha_t ce(x, t) w[i]
 * (targets t in [0, 1], weights w); with grad_out [n], out[i] <- grad_out[i] * d that / d logits[i]. */
int drc_focal_elementwise(int64_t n, const float* logits, const float* targets, const float* weights, float alpha, float gamma,
                          const float* grad_out, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * The frame change between the two networks (pts/frame_ops.hip; point_rcnn.py:296-312): the RPN's outputs, in the centred and rotated
 * frame of each instance cloud, back to the rectified camera frame.  One launch:
 *   xyz [B,N,3], boxes [B,M,7] as [x,y,z,h,w,l,ry], mean [B,3] fp32, rot [B] fp64 (the angle InstancePointCloud rotated the cloud by)
 *   xyz_cam [B,N,3] <- (p + mean) rotated about y by -rot; cos and sin of -rot are taken in fp64 and rounded once to fp32
 *   depth   [B,N]   <- |xyz_cam| with the rounding of drc_rpn_points_depth
 *   boxes_cam [B,M,7] <- the box through its corners as Box3DList does it, in fp32 and in that order: corners of the centred box, + mean,
 *                      the rotation, then centre = (c7 + c0) / 2, l, h, w = |c0 - c3|, |c0 - c1|, |c0 - c4|, ry = -atan2 of the edge 0 -> 3.
 *                      An all-zero padding box comes back as the rotated mean with zero size and ry = -0.0.
 * Nothing is launched when B = 0 or N = M = 0; with only one of N, M zero the other part is still written. */
int drc_rpn_to_camera_fwd(int B, int N, int M, const float* xyz, const float* boxes, const float* mean, const double* rot, float* xyz_cam,
                          float* depth, float* boxes_cam, void* stream);

/* drc_camera_to_rpn_fwd (frame_ops_train.hip): its twin, the way in.  xyz [B,K,3] camera-frame points of cloud b -> out [B,K,3] in that cloud's frame: times
 * `scale`, x negated when `flip`, rotated about y by rot[b] (fp64, the signed angle of the gather kernel), minus mean[b]. */
int drc_camera_to_rpn_fwd(int B, int K, const float* xyz, float scale, int flip, const float* mean, const double* rot, float* out,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * KITTI object scoring (pts/kitti_eval.hip; the KITTI devkit's evaluate_object.cpp): 2D, AOS, BEV and 3D precision at 41 recall samples.
 * ALL arithmetic and all floating-point buffers here are fp64, as the devkit's.
 *
 * Ragged input in CSR form over F frames: frame f owns ground-truth rows gt_off[f] .. gt_off[f+1] (DontCare rows included), detections
 * det_off[f] .. det_off[f+1] and the G_f * D_f pairs pair_off[f] + g * D_f + d (gt_off, det_off [F+1] int32, pair_off [F+1] int64).
 *   gt  [NG,14]: truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry      gt_cls  [NG] int32: 0 the class under
 *   det [ND,13]: alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score                       evaluation, 1 its neighbour class (Van for
 *   Car, Person_sitting for Pedestrian), 2 DontCare, 3 any other; det_cls [ND] int32: 0 the class under evaluation, 1 any other.
 * Per-frame limits: at most drc_kitti_eval_max_det() = 256 detections (the assigned-detection set is a bit mask of 4 x 64 bits) and
 * drc_kitti_eval_max_gt() = 4096 ground-truth rows.  The caller passes the largest per-frame counts (max_gt, max_det), which it knows
 * from the offsets it built; beyond the limits the status is -3 and nothing is launched.
 * Indices below: d = difficulty (easy, moderate, hard), m = metric (0 image, 1 ground, 2 3d), t = recall sample 0..40; metric_mask bit m
 * set = metric m is evaluated (the others are neither computed nor written, except where stated).
 * ------------------------------------------------------------------------------------- */
int drc_kitti_eval_max_det(void);
int drc_kitti_eval_max_gt(void);
/* cleanData: gt_ign [3,NG], det_ign [3,ND] int8 <- 0 valid, 1 ignored (may absorb a match without counting), -1 skipped */
int drc_kitti_eval_clean(int NG, int ND, const double* gt, const int32_t* gt_cls, const double* det, const int32_t* det_cls,
                         int8_t* gt_ign, int8_t* det_ign, void* stream);
/* ov [3,NP] <- per pair the image IoU, the rotated BEV IoU (centre t1, t3; extents l, w; angle ry) and the 3D IoU (BEV intersection times
 * the overlap of [t2 - h, t2]); for a DontCare row the intersection over the detection's own area / volume (the devkit's criterion 0). */
int drc_kitti_eval_overlaps(int F, int64_t NP, const double* gt, const int32_t* gt_cls, const double* det, const int32_t* gt_off,
                            const int32_t* det_off, const int64_t* pair_off, int metric_mask, double* ov, void* stream);
/* computeStatistics without false positives, one thread per (frame, d, m): matched [3,3,NG] int8 <- 1 where the ground-truth row counts
 * as a true positive (every element is written), v [3,3,NG] <- the score of its detection (written where matched is 1 only). */
int drc_kitti_eval_pass1(int F, int NG, int ND, int64_t NP, int max_gt, int max_det, const double* gt, const int32_t* gt_cls,
                         const double* det, const int32_t* gt_off, const int32_t* det_off, const int64_t* pair_off,
                         const int8_t* gt_ign, const int8_t* det_ign, const double* ov, int metric_mask, double min_overlap_image,
                         double min_overlap_ground, double min_overlap_3d, double* v, int8_t* matched, void* stream);
/* computeStatistics with false positives, one thread per (frame, d, m, t): thresholds [3,3,41], of which the first n_thresholds [3,3]
 * (int32) are used.  counts [3,3,41,3,F] int16 <- tp, fp, fn of each frame (the per-frame limits keep them below 2^15); sim [3,3,41,F] <- its orientation-similarity sum (metric 0
 * with compute_aos != 0; 0 for a frame without tp and fp).  Every element is written (0 for a metric or a sample that is not used). */
int drc_kitti_eval_pass2(int F, int NG, int ND, int64_t NP, int max_gt, int max_det, const double* gt, const int32_t* gt_cls,
                         const double* det, const int32_t* gt_off, const int32_t* det_off, const int64_t* pair_off,
                         const int8_t* gt_ign, const int8_t* det_ign, const double* ov, int metric_mask, double min_overlap_image,
                         double min_overlap_ground, double min_overlap_3d, int compute_aos, const double* thresholds,
                         const int32_t* n_thresholds, int16_t* counts, double* sim, void* stream);
/* out_counts [3,3,41,3] int64, out_sim [3,3,41] <- the sums over the frames, in an order that depends on F alone (no atomics):
 * bit-identical run to run. */
int drc_kitti_eval_reduce(int F, const int16_t* counts, const double* sim, int64_t* out_counts, double* out_sim, void* stream);

/* ---------------------------------------------------------------------------------------
 * The solver (solver.hip): gradient norm, clipping and the SGD / Adam update of ALL parameter tensors in three launches.
 *
 * The host builds the work table once (disprcnn_amd/solver/fused.py):
 *   tensors int64 [T,5]: parameter pointer, gradient pointer, offset into the flat state buffers (floats, a multiple of 4), numel, group
 *   chunks  int64 [C,2]: tensor, start (a multiple of drc_solver_chunk()); one workgroup per chunk, none for an empty tensor
 *   hyper   fp32  [G,8]: lr, weight_decay, momentum | beta1, beta2, eps, 1 - beta1, 1 - beta2, 0
 *   derived fp32  [G,2]: Adam's lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t), written by drc_solver_prepare
 *   scalars fp32  [4]  : total_norm, clip_coef, the step count as a float, 0;   step int64 [1]: the step count
 * Parameters and gradients need 4-byte alignment only.  Every sum has a fixed order: bit-identical run to run.
 * ------------------------------------------------------------------------------------- */
int drc_solver_chunk(void);
/* partials [C] fp64 <- the sum of g^2 over each chunk */
int drc_solver_grad_norm(int64_t n_chunks, int64_t n_tensors, const int64_t* tensors, const int64_t* chunks, double* partials,
                         void* stream);
/* flags: 1 = add the partials in chunk order, write total_norm and clip_coef = min(1, max_norm / (total_norm + 1e-6));
 *        2 = leave clip_coef as an earlier call wrote it (without 1 and 2 it becomes 1);
 *        4 = advance the step count and, for Adam, write `derived` for the new count. */
int drc_solver_prepare(int64_t n_chunks, const double* partials, int flags, float max_norm, int n_groups, int adam, const float* hyper,
                       float* derived, float* scalars, int64_t* step, void* stream);
/* torch.optim.SGD (dampening 0, no Nesterov): d = g + wd * p; buf = momentum * buf + d; p -= lr * buf.  momentum_buf may be null
 * (momentum 0).  clip != 0: g is scaled by clip_coef first and written back, as clip_grad_norm_ leaves it. */
int drc_solver_sgd_step(int64_t n_chunks, int64_t n_tensors, int n_groups, const int64_t* tensors, const int64_t* chunks,
                        const float* hyper, const float* scalars, float* momentum_buf, int clip, void* stream);
/* torch.optim.Adam (no amsgrad, L2 weight decay on the gradient), bias correction from `derived` */
int drc_solver_adam_step(int64_t n_chunks, int64_t n_tensors, int n_groups, const int64_t* tensors, const int64_t* chunks,
                         const float* hyper, const float* derived, const float* scalars, float* exp_avg, float* exp_avg_sq, int clip,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * Training targets, balanced sampling and losses of the stereo 2D stage (det_train.hip; reference modeling/rpn/stereo_rpn/loss.py,
 * roi_heads/box_head/loss.py, matcher.py, balanced_positive_negative_sampler.py, box_coder.py encode_*, utils/stereo_utils.py
 * expand_left_right_box).  All images go in one launch: `cand_off` / `gt_off` are HOST arrays of N + 1 int32 CSR offsets (first 0,
 * ascending) of the images' candidates and ground truths; N <= DRC_DET2D_MAX_IMAGES.  Decisions are fp32 in the reference's order, loss
 * sums fp64 (per-block partials added in block order: bit-identical run to run).  No entry synchronises or reads back.
 *
 * drc_det2d_match_fwd -- boxlist_iou + Matcher(high, low, allow_low_quality) + labels + BoxCoder.encode for every candidate.
 *   cand [R,cs]: cs = 4 anchors (xyxy) or cs = 6 joint proposals (x1 y1 x2 y2 x1' x2'; matched by the union of their two views and
 *   encoded ..._fromboxes6); gt_left / gt_right [G,4]: the two views of the ground truths, matched by their union box and encoded from
 *   original_lr_bbox = (left x1, union y1, left x2, union y2, right x1, right x2).  1 .. DRC_DET2D_MAX_GT ground truths and at least one
 *   candidate per image, else -2.  Ties of the per-candidate maximum go to the lowest row.  allow_low_quality: gt_max [G] uint32 of
 *   workspace receives each ground truth's largest IoU (an integer maximum of the bit patterns: order-free), and every candidate whose
 *   IoU with a ground truth equals it keeps its best row (set_low_quality_matches_, ties and a maximum of 0 included).
 *   matched [R] int64 = row within the image, -1 below `low`, -2 below `high`.  Label: gt_labels [G] int64 at the row clamped at 0, or 1
 *   without gt_labels; 0 where matched is -1; -1 where it is -2 or where visibility [R] u8 (optional) is 0.  It is written as fp32
 *   and / or int64, whichever pointers are given.  reg_targets [R,6] = (dx, dy, dw, dh, dx', dw') with weights4 = (wx, wy, ww, wh).
 * drc_det2d_sample_fwd -- BalancedPositiveNegativeSampler with the randomness as an input: per image num_pos = min(#positives,
 *   cap_pos), num_neg = min(#negatives, batch - num_pos); the members with the smallest (draws[i], i) keys are taken (radix select on
 *   the bit pattern of the draw, draws >= 0; one workgroup per image and class).  labels: label_kind 0 fp32, 1 int64 (>= 1 positive, 0
 *   negative, else ignored).  pos_mask / neg_mask [R] u8, counts [N,2] int32 = (num_pos, num_neg); sampled_idx (optional) [N,batch]
 *   int64 = the image-local indices of pos | neg in ascending order, -1 past the count.
 * drc_det2d_srpn_loss_fwd -- SRPNLossComputation's two losses and their gradients with respect to the RAW head maps.  levels: HOST
 *   int64 [n_levels,7] = cls_logits [N,2A,H,W], bbox_pred [N,6A,H,W], grad of each (same shapes, every element written), H, W, offset of
 *   the level's first anchor within an image (levels in order, anchors position-major: (y*W + x)*A + a); `total` anchors per image;
 *   masks [N*total] as the sampler wrote them, reg_targets [N*total,6], counts [N,2].  The head's softmax pairs raw channel c with
 *   c + A (srpn.py:47); the loss reads the probability map as (A,2): anchor a's vector is (p[2a], p[2a+1]) and the objective is
 *   cross_entropy of THAT vector (a log-softmax of probabilities).  terms [3] = loss_objectness (mean over the sampled anchors),
 *   loss_rpn_box_reg (smooth L1 with `beta` over the sampled positives' six codes, summed, over the sampled count), the count;
 *   with no sampled anchor both losses and every gradient are 0.  partials: drc_det2d_srpn_loss_partials(...) doubles.
 * drc_det2d_fastrcnn_loss_fwd -- cross_entropy(class_logits [R,C], labels [R] int64) and smooth L1 (beta 1) over columns 6*label ..
 *   6*label+5 of box_regression [R,6C] against reg_targets [R,6] on rows with label > 0, both over R.  terms [3] = the two losses, R;
 *   grad_logits / grad_box: every element written.  partials: 2 * ceil(R / 256) doubles.
 * drc_det2d_mask_loss_fwd -- project_masks_on_boxes + binary_cross_entropy_with_logits of the mask head, one workgroup per ROI.  roi_off /
 *   inst_off: HOST CSR offsets of the images' ROIs and instances.  boxes [P,4] xyxy; matched [P] int64 as drc_det2d_match_fwd wrote it
 *   (no low-quality matches); inst_labels [I] int64; mask_logits [P,C,M,M]; masks: the instances' uint8 0/1 maps in one flat buffer,
 *   table [I,3] int64 (device) = offset, H, W of each.  A ROI is positive when its match is not -1 and the instance at the matched row
 *   clamped at 0 has a label in (0, C); the others drop out on the device (zero target, zero gradient).  Crop as BinaryMaskList.crop
 *   (round half to even of the fp32 coordinate in double, the four clamps, at least one pixel), bilinear resize to M x M in the
 *   arithmetic of torch's CPU upsample_bilinear2d (align_corners = False; mask_resize.h), truncated to uint8: 1 only where the value
 *   reaches 1.0.  targets [P,M,M] u8; count [1] int32 = positive ROIs; terms [2] = the mean over their pixels of max(x,0) - x*t +
 *   log1p(exp(-|x|)) (0 without a positive ROI), the pixel count; grad_logits [P,C,M,M] = (sigmoid(x) - t) / pixels on the ROI's class
 *   plane, 0 elsewhere, every element written.  partials: P doubles.
 * ------------------------------------------------------------------------------------- */
#define DRC_DET2D_MAX_IMAGES 64
#define DRC_DET2D_MAX_GT 128
#define DRC_DET2D_MAX_LEVELS 8
int drc_det2d_max_gt(void);
int drc_det2d_max_images(void);
int drc_det2d_match_fwd(int N, const int32_t* cand_off, const int32_t* gt_off, int cs, const float* cand, const float* gt_left,
                        const float* gt_right, const int64_t* gt_labels, const uint8_t* visibility, float high, float low,
                        int allow_low_quality, const float* weights4, uint32_t* gt_max, int64_t* matched, float* labels_f32,
                        int64_t* labels_i64, float* reg_targets, void* stream);
int drc_det2d_sample_fwd(int N, const int32_t* cand_off, const void* labels, int label_kind, const float* draws, int batch, int cap_pos,
                         uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts, int64_t* sampled_idx, void* stream);
int64_t drc_det2d_srpn_loss_partials(int N, int A, int n_levels, const int64_t* levels);
int drc_det2d_srpn_loss_fwd(int N, int A, int n_levels, const int64_t* levels, int64_t total, const uint8_t* pos_mask,
                            const uint8_t* neg_mask, const float* reg_targets, const int32_t* counts, double beta, double* partials,
                            float* terms, void* stream);
int drc_det2d_fastrcnn_loss_fwd(int R, int C, const float* class_logits, const int64_t* labels, const float* box_regression,
                                const float* reg_targets, float* grad_logits, float* grad_box, double* partials, float* terms,
                                void* stream);
int drc_det2d_mask_loss_fwd(int N, const int32_t* roi_off, const int32_t* inst_off, int C, int M, const float* boxes,
                            const int64_t* matched, const int64_t* inst_labels, const float* mask_logits, const uint8_t* masks,
                            const int64_t* table, int32_t* count, uint8_t* targets, float* grad_logits, double* partials, float* terms,
                            void* stream);

/* -------------------------------------------------------------------------------------
 * ResNet body training (body_train.hip): the weight gradient of a 1x1 convolution as a GEMM over pixels.
 *
 * drc_conv1x1_wgrad_blocked -- gw[co][ci] = sum_{n,y,x} b[n,co,y,x] * a[n,ci,s*y,s*x], s = stride in {1, 2}.  a and b are blocked fp32
 *   tensors float[N][CB][H+2ph][W+2pw][16] of any halo, each given as its strides in floats (unit, channel block, row) and the offset of
 *   its interior's first element inside a (unit, channel block); b's interior is OH x OW, a's must reach (s*(OH-1), s*(OW-1)).  cin / cout
 *   are the UNPADDED channel counts: gw is dense fp32 [cout][cin], every element overwritten, and the padded channels of a last block do
 *   not reach it.  The flat pixel index is cut into chunks of `chunk` pixels (> 0): fp32 (v_mfma_f32_16x16x4_f32) within a chunk,
 *   partials [chunks][cout][cin] to scratch, a finishing launch adds them in chunk order in fp64 and rounds once.  No atomics; the bits
 *   depend on the operands and on `chunk` only.  N = 0: zeros.  scratch_floats < drc_conv1x1_wgrad_scratch_floats(...): -3.
 * ------------------------------------------------------------------------------------- */
int drc_conv1x1_wgrad_default_chunk(void);
int64_t drc_conv1x1_wgrad_scratch_floats(int N, int OH, int OW, int cin, int cout, int chunk);
int drc_conv1x1_wgrad_blocked(const float* a, int64_t a_n_stride, int64_t a_cb_stride, int64_t a_h_stride, int64_t a_off0,
                              const float* b, int64_t b_n_stride, int64_t b_cb_stride, int64_t b_h_stride, int64_t b_off0,
                              int N, int OH, int OW, int cin, int cout, int stride, int chunk, float* gw, float* scratch,
                              int64_t scratch_floats, void* stream);

/* -------------------------------------------------------------------------------------
 * Input pipeline (input_ops.hip): decoded uint8 images -> the padded fp32 batch of an ImageList; resize / flip of instance masks.
 *
 * drc_input_batch_fwd -- out fp32 [I,3,Hp,Wp]: out[i][c][y][x] = lut[c][ src_i[ytab_i[y]][xtab_i[x]][chan_c] ] for y < out_h_i and
 *   x < out_w_i, +0.0 elsewhere.  Every element, padding included, is written exactly once (no memset; `out` may be uninitialised and
 *   needs 4-byte alignment only: whole quads are 16-byte stores, the clipped first / last quad goes element by element).
 *   src: packed uint8 HWC RGB images, src_bytes long.  tables: int32, table_ints long: I descriptors of 8 ints (src_off into src, src_h,
 *   src_w, out_h, out_w, ytab_off, xtab_off into tables, 0) followed by the index tables (out_h + out_w entries per image; they carry
 *   the resize and the flip).  lut: fp32 [3][256].  chan0..2: the source channel of each output channel, in 0..2.  Table positions,
 *   table entries and byte indices are clamped into their buffers.  The grid is min(quads / 256, max_blocks) workgroups that stride;
 *   drc_input_default_max_blocks() is what the callers pass.  I = 0 or an empty plane: nothing is launched.  Hp * Wp >= 2^31: -2.
 *
 * drc_mask_resize_flip_fwd -- n_jobs jobs of drc_mask_job_cols() int64 each, on the device: src pointer (uint8 [G,H,W], 0/1), dst pointer
 *   (uint8 [G,oh,ow]), G, H, W, oh, ow, flip, first quad, quads (= ceil(G*oh*ow / 4)); first quads ascend from 0 and sum to `quads`; jobs
 *   without output are left out by the caller.  Taps and weights of mask_resize.h:resize_axis; a pixel is 1 iff every tap whose fp32
 *   weight is non-zero is 1 (the truncated bilinear blend in exact arithmetic; no floating-point sum).  flip: column x reads the resized
 *   column ow-1-x.  Equal sizes copy (or flip) exactly.  n_jobs = 0 or quads = 0: nothing is launched.
 * ------------------------------------------------------------------------------------- */
int drc_input_default_max_blocks(void);
int drc_input_batch_fwd(const uint8_t* src, int64_t src_bytes, const int32_t* tables, int64_t table_ints, const float* lut, int chan0,
                        int chan1, int chan2, int I, int Hp, int Wp, float* out, int max_blocks, void* stream);
int drc_mask_job_cols(void);
int drc_mask_resize_flip_fwd(const int64_t* jobs, int n_jobs, int64_t quads, int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DISPRCNN_PTS_H */
