// Registration of image sequences: every frame, with its own observer, grid and time, resampled onto one
// reference observer, grid and time through the sphere r = radius and a three-term differential rotation law.
// Conventions, formulas and argument rules: include/sunerf_hip_register.h.  All geometry is fp64; the only fp32 values are the
// poses read and the results stored.
//   register_frames_kernel<order>   one launch for all frames: grid (tiles along x, tiles along y, frames), one workgroup per
//                                   16 x 16 output pixels so that its taps fall in a compact part of the source, one lane per
//                                   pixel.  The sines and cosines of the tile's 16 + 16 reference angles are formed once (LDS); the
//                                   map and the 2 (order + 1) weights are formed once per pixel and reused over the planes;
//                                   the frame's descriptor is wave-uniform and is read through the scalar cache.
// The tap sum is prep_math.h's (the same statements as prep_sample, with the weights hoisted out of the plane loop); axis_coord
// and inverse_rotate are reprojection.hip's (reproject_math.h).  The four counters of a frame are integer atomics: LDS first,
// one global add per counter and workgroup.  The only data-dependent loops are the two bisections, bounded by the axis length.
#include "sunerf_common.h"
#include "prep_math.h"
#include "reproject_math.h"
#include "../../include/sunerf_hip_register.h"

namespace {

constexpr int kTile = SUNERF_REGISTER_TILE;
constexpr double kEdgeEps = SUNERF_REGISTER_EDGE_EPS;

struct RegisterArgs {
  const SunerfRegisterFrameDesc* frames;
  int n_planes;
  const float* c2w_ref; const double* tx_ref; const double* ty_ref;
  int H, W;
  double R, A, B, C;
  int closest; float missing; int propagate;
  float* out; uint8_t* status; double* coords; unsigned long long* state;
};

// step 6 of the header: the coordinate on the border when it is within kEdgeEps outside it
__device__ __forceinline__ double snap_edge(double v, int n) {
  const double last = (double)(n - 1);
  if (v < 0. && v >= -kEdgeEps) return 0.;
  if (v > last && v <= last + kEdgeEps) return last;
  return v;
}

template <int order>
__global__ __launch_bounds__(kTile * kTile) void register_frames_kernel(RegisterArgs a) {
  __shared__ unsigned tally[SUNERF_REGISTER_STATE];
  __shared__ double trig[4][kTile];      // sin Tx, cos Tx of the tile's columns, sin Ty, cos Ty of its rows
  const int t = threadIdx.x, k = blockIdx.z;
  if (t < SUNERF_REGISTER_STATE) tally[t] = 0u;
  // the tile's 16 + 16 angles are the same for its 256 pixels: 16 lanes of the first wave take the columns, 16 of the second the rows
  if (t < kTile) {
    const int col = blockIdx.x * kTile + t;
    const double Tx = col < a.W ? a.tx_ref[col] : 0.;
    trig[0][t] = sin(Tx); trig[1][t] = cos(Tx);
  } else if (t >= 64 && t < 64 + kTile) {
    const int row = blockIdx.y * kTile + (t - 64);
    const double Ty = row < a.H ? a.ty_ref[row] : 0.;
    trig[2][t - 64] = sin(Ty); trig[3][t - 64] = cos(Ty);
  }
  __syncthreads();
  const int r = blockIdx.y * kTile + (t >> 4), c = blockIdx.x * kTile + (t & 15);
  if (r < a.H && c < a.W) {
    const SunerfRegisterFrameDesc& f = a.frames[k];
    const int h = f.height, w = f.width;
    const bool usable = f.coefficients != nullptr && h >= 1 && w >= 1;
    double cy = quiet_nan(), cx = quiet_nan();
    int status;
    bool sample = false;
    {
      // 1: the line of sight of the reference pixel
      const double sx = trig[0][t & 15], cTx = trig[1][t & 15], sy = trig[2][t >> 4], cTy = trig[3][t >> 4];
      const double e[3] = {sx, -sy * cTx, -cTx * cTy};
      double o[3], d[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        d[i] = ((double)a.c2w_ref[4 * i] * e[0] + (double)a.c2w_ref[4 * i + 1] * e[1]) + (double)a.c2w_ref[4 * i + 2] * e[2];
        o[i] = (double)a.c2w_ref[4 * i + 3];
      }
      const double v0 = o[1] * d[2] - o[2] * d[1], v1 = o[2] * d[0] - o[0] * d[2], v2 = o[0] * d[1] - o[1] * d[0];
      const double R2 = a.R * a.R;
      const double m = R2 - ((v0 * v0 + v1 * v1) + v2 * v2);
      const double od = (o[0] * d[0] + o[1] * d[1]) + o[2] * d[2];
      const bool on_disk = m > 0. && od < 0.;
      status = on_disk ? SUNERF_REGISTER_ON_DISK : SUNERF_REGISTER_OFF_DISK;
      if (on_disk || a.closest) {
        // 2, 3: the scene point and where it was when the frame was taken
        const double s = on_disk ? -od - sqrt(m) : -od;
        const double p0 = o[0] + d[0] * s, p1 = o[1] + d[1] * s, p2 = o[2] + d[2] * s;
        const double rho = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
        const double lat = atan2(-p2, hypot(p0, p1)), lon = atan2(-p0, p1);
        const double sl = sin(lat), cl = cos(lat);
        const double s2 = sl * sl;
        const double rate = (a.A + a.B * s2) + a.C * (s2 * s2);
        const double lon_k = lon + rate * f.dt;
        double q[3] = {rho * (-cl * sin(lon_k)), rho * (cl * cos(lon_k)), rho * (-sl)};
        // 4: visibility from the frame's observer
        const double ok0 = (double)f.c2w[3], ok1 = (double)f.c2w[7], ok2 = (double)f.c2w[11];
        const double margin = ((q[0] * ok0 + q[1] * ok1) + q[2] * ok2) - R2;
        if (on_disk && !(margin > 0.)) {
          status = SUNERF_REGISTER_BEHIND;
        } else if (!usable) {
          status = SUNERF_REGISTER_OUTSIDE;
        } else {
          // 5, 6: the frame's pixel
          double cam[3];
          q[0] -= ok0; q[1] -= ok1; q[2] -= ok2;
          inverse_rotate(f.c2w, q, cam);
          const double Txk = atan2(cam[0], hypot(cam[1], cam[2]));
          const double Tyk = atan2(-cam[1], -cam[2]);
          cx = axis_coord(f.tx, w, Txk) + f.shift_x;
          cy = axis_coord(f.ty, h, Tyk) + f.shift_y;
          const double ey = snap_edge(cy, h), ex = snap_edge(cx, w);
          sample = ey >= 0. && ey <= (double)(h - 1) && ex >= 0. && ex <= (double)(w - 1);      // false for NaN
          if (sample) { cy = ey; cx = ex; } else status = SUNERF_REGISTER_OUTSIDE;
        }
      }
    }
    const int64_t plane_out = (int64_t)a.H * a.W, at = (int64_t)r * a.W + c;
    a.status[(int64_t)k * plane_out + at] = (uint8_t)status;
    if (a.coords) {
      double* co = a.coords + (int64_t)k * 2 * plane_out;
      co[at] = cy; co[plane_out + at] = cx;
    }
    atomicAdd(&tally[status == SUNERF_REGISTER_ON_DISK ? 0 : status == SUNERF_REGISTER_OFF_DISK ? 1
                     : status == SUNERF_REGISTER_BEHIND ? 2 : 3], 1u);
    float* out = a.out + (int64_t)k * a.n_planes * plane_out + at;
    if (!sample) {
      for (int pl = 0; pl < a.n_planes; ++pl) out[pl * plane_out] = a.missing;
    } else {
      // 7: prep_sample's tap sum, weights and indices formed once for all planes
      const int64_t sy0 = prep_start(cy, order), sx0 = prep_start(cx, order);
      double wy[order + 1], wx[order + 1];
      int64_t iy[order + 1];
      int ix[order + 1];
      if (order > 0) {
        prep_weights(cy, order, wy);
        prep_weights(cx, order, wx);
      }
#pragma unroll
      for (int j = 0; j <= order; ++j) {
        iy[j] = (int64_t)prep_mirror(sy0 + j, h) * w;
        ix[j] = prep_mirror(sx0 + j, w);
      }
      const int64_t plane_in = (int64_t)h * w;
      const bool masked = a.propagate && f.mask != nullptr;
      for (int pl = 0; pl < a.n_planes; ++pl) {
        const double* coef = f.coefficients + pl * plane_in;
        const uint8_t* mask = masked ? f.mask + pl * plane_in : nullptr;
        double sum = 0.0;
        bool hit = false;
#pragma unroll
        for (int i = 0; i <= order; ++i) {
#pragma unroll
          for (int j = 0; j <= order; ++j) {
            double v = coef[iy[i] + ix[j]];
            if (masked && mask[iy[i] + ix[j]]) hit = true;
            if (order > 0) {
              v *= wy[i];
              v *= wx[j];
            }
            sum += v;
          }
        }
        out[pl * plane_out] = hit ? __int_as_float(0x7fc00000) : (float)sum;
      }
    }
  }
  __syncthreads();
  if (t < SUNERF_REGISTER_STATE && tally[t]) atomicAdd(a.state + (int64_t)blockIdx.z * SUNERF_REGISTER_STATE + t, (unsigned long long)tally[t]);
}

template <int order>
void launch(const RegisterArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(register_frames_kernel<order>, grid, dim3(kTile * kTile), 0, st, a);
}

}  // namespace

extern "C" int sunerf_register_abi_version(void) { return SUNERF_REGISTER_ABI_VERSION; }

extern "C" size_t sunerf_register_frame_desc_bytes(void) { return sizeof(SunerfRegisterFrameDesc); }

extern "C" int sunerf_register_frames(const SunerfRegisterFrameDesc* frames, int n_frames, int n_planes, int order,
                                      const float* c2w_ref, const double* tx_ref, const double* ty_ref, int out_height, int out_width,
                                      double radius, double A, double B, double C, int off_disk, float missing, int flags, float* out,
                                      uint8_t* status, double* coords, int64_t* state, void* stream) {
  if (order < 0 || order > SUNERF_PREP_MAX_ORDER) return SUNERF_E_UNSUPPORTED;
  if (off_disk != SUNERF_REGISTER_OFF_DISK_MISSING && off_disk != SUNERF_REGISTER_OFF_DISK_CLOSEST) return SUNERF_E_UNSUPPORTED;
  if (flags & ~SUNERF_REGISTER_PROPAGATE) return SUNERF_E_UNSUPPORTED;
  const bool negative = n_frames < 0 || n_planes < 0 || out_height < 0 || out_width < 0;
  if (!negative && (n_frames == 0 || out_height == 0 || out_width == 0)) return 0;
  if (negative || n_planes == 0 || n_frames > 65535 || out_height > kTile * 65535) return SUNERF_E_BADARG;      // grid y and z
  if (!finite_positive(radius) || !is_finite(A) || !is_finite(B) || !is_finite(C)) return SUNERF_E_BADARG;
  if (!frames || !c2w_ref || !tx_ref || !ty_ref || !out || !status || !state) return SUNERF_E_BADARG;
  if ((uintptr_t)frames % 8 || (uintptr_t)tx_ref % 8 || (uintptr_t)ty_ref % 8 || (uintptr_t)coords % 8 || (uintptr_t)state % 8)
    return SUNERF_E_BADARG;
  if ((uintptr_t)c2w_ref % 4 || (uintptr_t)out % 4) return SUNERF_E_BADARG;
  RegisterArgs a;
  a.frames = frames; a.n_planes = n_planes; a.c2w_ref = c2w_ref; a.tx_ref = tx_ref; a.ty_ref = ty_ref;
  a.H = out_height; a.W = out_width; a.R = radius; a.A = A; a.B = B; a.C = C;
  a.closest = off_disk == SUNERF_REGISTER_OFF_DISK_CLOSEST; a.missing = missing; a.propagate = flags & SUNERF_REGISTER_PROPAGATE;
  a.out = out; a.status = status; a.coords = coords; a.state = reinterpret_cast<unsigned long long*>(state);
  hipStream_t st = (hipStream_t)stream;
  const unsigned tiles_y = (unsigned)((out_height + kTile - 1) / kTile), tiles_x = (unsigned)((out_width + kTile - 1) / kTile);
  SUNERF_CLEAR_ERROR();
  hipError_t e = hipMemsetAsync(state, 0, (size_t)n_frames * SUNERF_REGISTER_STATE * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(tiles_x, tiles_y, (unsigned)n_frames);
  switch (order) {
    case 0: launch<0>(a, grid, st); break;
    case 1: launch<1>(a, grid, st); break;
    case 2: launch<2>(a, grid, st); break;
    case 3: launch<3>(a, grid, st); break;
    case 4: launch<4>(a, grid, st); break;
    default: launch<5>(a, grid, st); break;
  }
  SUNERF_CHECK_LAUNCH();
  return 0;
}
