// ctypes binding for the reference's own PointNet++ GPU kernels (pointnet2_lib/pointnet2/src/*_gpu.cu), compiled for gfx950 by
// oracle/build_pn2_ref.py into oracle/_ref/libpn2_ref.so.  Test infrastructure only: it pins disprcnn_amd/pts/pointnet2.hip and
// tests/pn2_oracle.py against the kernels they restate; nothing in the product path loads it.
//
// The reference's launchers are declared here by their signatures (its headers also declare the torch-facing wrappers, which are
// not built).  Every entry takes device pointers, launches on the null stream and waits, so a fault surfaces at the call that made
// it.  The reference kernels do no bounds checks: callers pass in-range indices only, and keep grid y / z (c, b) <= 65535.
#include <hip/hip_runtime.h>

void furthest_point_sampling_kernel_launcher(int b, int n, int m, const float* dataset, float* temp, int* idxs, hipStream_t stream);
void gather_points_kernel_launcher_fast(int b, int c, int n, int npoints, const float* points, const int* idx, float* out,
                                        hipStream_t stream);
void gather_points_grad_kernel_launcher_fast(int b, int c, int n, int npoints, const float* grad_out, const int* idx, float* grad_points,
                                             hipStream_t stream);
void ball_query_kernel_launcher_fast(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int* idx,
                                     hipStream_t stream);
void group_points_kernel_launcher_fast(int b, int c, int n, int npoints, int nsample, const float* points, const int* idx, float* out,
                                       hipStream_t stream);
void group_points_grad_kernel_launcher_fast(int b, int c, int n, int npoints, int nsample, const float* grad_out, const int* idx,
                                            float* grad_points, hipStream_t stream);
void three_nn_kernel_launcher_fast(int b, int n, int m, const float* unknown, const float* known, float* dist2, int* idx,
                                   hipStream_t stream);
void three_interpolate_kernel_launcher_fast(int b, int c, int m, int n, const float* points, const int* idx, const float* weight,
                                            float* out, hipStream_t stream);
void three_interpolate_grad_kernel_launcher_fast(int b, int c, int n, int m, const float* grad_out, const int* idx, const float* weight,
                                                 float* grad_points, hipStream_t stream);

namespace {
int done() { return (int)hipDeviceSynchronize(); }
}  // namespace

extern "C" {

int pn2_ref_furthest_point_sampling(int b, int n, int m, const float* xyz, float* temp, int* idx) {
    furthest_point_sampling_kernel_launcher(b, n, m, xyz, temp, idx, nullptr);
    return done();
}

int pn2_ref_gather_points(int b, int c, int n, int npoints, const float* points, const int* idx, float* out) {
    gather_points_kernel_launcher_fast(b, c, n, npoints, points, idx, out, nullptr);
    return done();
}

int pn2_ref_gather_points_grad(int b, int c, int n, int npoints, const float* grad_out, const int* idx, float* grad_points) {
    gather_points_grad_kernel_launcher_fast(b, c, n, npoints, grad_out, idx, grad_points, nullptr);
    return done();
}

int pn2_ref_ball_query(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int* idx) {
    ball_query_kernel_launcher_fast(b, n, m, radius, nsample, new_xyz, xyz, idx, nullptr);
    return done();
}

int pn2_ref_group_points(int b, int c, int n, int npoints, int nsample, const float* points, const int* idx, float* out) {
    group_points_kernel_launcher_fast(b, c, n, npoints, nsample, points, idx, out, nullptr);
    return done();
}

int pn2_ref_group_points_grad(int b, int c, int n, int npoints, int nsample, const float* grad_out, const int* idx, float* grad_points) {
    group_points_grad_kernel_launcher_fast(b, c, n, npoints, nsample, grad_out, idx, grad_points, nullptr);
    return done();
}

int pn2_ref_three_nn(int b, int n, int m, const float* unknown, const float* known, float* dist2, int* idx) {
    three_nn_kernel_launcher_fast(b, n, m, unknown, known, dist2, idx, nullptr);
    return done();
}

int pn2_ref_three_interpolate(int b, int c, int m, int n, const float* points, const int* idx, const float* weight, float* out) {
    three_interpolate_kernel_launcher_fast(b, c, m, n, points, idx, weight, out, nullptr);
    return done();
}

int pn2_ref_three_interpolate_grad(int b, int c, int n, int m, const float* grad_out, const int* idx, const float* weight,
                                   float* grad_points) {
    three_interpolate_grad_kernel_launcher_fast(b, c, n, m, grad_out, idx, weight, grad_points, nullptr);
    return done();
}

}  // extern "C"
