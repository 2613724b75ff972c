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

#ifdef __cplusplus
}
#endif

#endif /* DISPRCNN_PTS_H */
