// Mel-cepstral distortion along a dynamic-time-warping path (gsttaco_mel_dtw, include/gsttaco.h): the free-run metric.  Off the mel-frame
// hot path; double throughout after the fp32 load.
//
//   gt_dtw_features_kernel   one thread per feature of a frame of x or y: clip to the normalisation's range, to double, (the DCT-II row
//                            of the coefficient over the channels in ascending channel order, or the channel itself), times the dB scale.
//                            ONE device function serves both sides, so equal inputs give bitwise equal features and a distance of
//                            exactly 0.  Frames at or beyond a row's length are not read and their features not written.  Features lie [b][k][t].
//   gt_dtw_align_kernel      one workgroup per utterance sweeps the anti-diagonals d = i + j of D(i,j) = C(i,j) + min(diagonal, up, left).
//                            Column j belongs to thread j mod GT_DTW_THREADS (a thread loops over its columns, so Ly may exceed the
//                            workgroup).  Three rolling diagonals of D and of the path length live in LDS, indexed by the column and
//                            sized by Ty: cell (i,j) reads up = [d-1][j], left = [d-1][j-1], diagonal = [d-2][j-1] and writes [d][j];
//                            the buffer written at d was last read at d - 1, so ONE barrier per diagonal orders everything.  C(i,j) is
//                            computed on the fly from the two feature rows; nothing of size Lx * Ly exists except the optional
//                            back-pointers (one byte per cell, written only when the caller asks for the path).  The path length is
//                            carried with the chosen predecessor.  Behind the sweep the same launch fills the path rows with -1 and
//                            thread 0 walks the back-pointers from (Lx-1, Ly-1), writing row len-1 down to row 0.
// Every loop is bounded by the row's clipped lengths (a NaN only ever loses a comparison), every global access by them too, and no
// workgroup waits on another.  No floating-point atomics: a call is bitwise reproducible.
#include <algorithm>

#include "kernels.h"
#include "device_utils.h"

#define GT_DTW_THREADS 1024
#define GT_DTW_FEAT_THREADS 256

__device__ __forceinline__ int gt_dtw_len(const int32_t* len, int b, int T) { return len ? min(max((int)len[b], 0), T) : T; }

// One feature of one frame (`fr`: its M channels): the shared code path of both sides.
__device__ __forceinline__ double gt_dtw_feature(const float* fr, int k, int M, int n_ceps, const double* basis, float lo, float hi,
                                                 double scale) {
    auto value = [&](int m) {
        const float v = fr[m];
        if (!isfinite(v)) return (double)NAN;                   // (a clip would turn an infinity into an ordinary value)
        return (double)(v < lo ? lo : v > hi ? hi : v);
    };
    if (n_ceps == 0) return value(k) * scale;
    const double* row = basis + (int64_t)k * M;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += value(m) * row[m];
    return s * scale;
}

__global__ __launch_bounds__(GT_DTW_FEAT_THREADS) void gt_dtw_features_kernel(DtwArgs P) {
    const int F = P.n_ceps ? P.n_ceps : P.mel_dim;
    const int64_t nx = (int64_t)P.B * P.Tx * F, n = nx + (int64_t)P.B * P.Ty * F;
    for (int64_t e = (int64_t)blockIdx.x * GT_DTW_FEAT_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * GT_DTW_FEAT_THREADS) {
        const bool is_y = e >= nx;
        const int64_t q = is_y ? e - nx : e;
        const int T = is_y ? P.Ty : P.Tx;
        const int k = (int)(q % F);
        const int t = (int)((q / F) % T), b = (int)(q / ((int64_t)F * T));
        if (t >= gt_dtw_len(is_y ? P.y_len : P.x_len, b, T)) continue;
        const float* fr = (is_y ? P.y + (int64_t)b * P.y_stride : P.x + (int64_t)b * P.x_stride) + (int64_t)t * P.mel_dim;
        // [b][k][t]: the sweep's lanes own adjacent columns / rows, so one feature of adjacent frames is one contiguous read there
        (is_y ? P.fy : P.fx)[((int64_t)b * F + k) * T + t] = gt_dtw_feature(fr, k, P.mel_dim, P.n_ceps, P.basis, P.clip_lo, P.clip_hi, P.scale);
    }
}

__global__ __launch_bounds__(GT_DTW_THREADS) void gt_dtw_align_kernel(DtwArgs P) {
    extern __shared__ double dtw_lds[];                         // [3][Ty] D, then [3][Ty] int32 path lengths
    const int Ty = P.Ty, Tx = P.Tx;
    double* Dd = dtw_lds;
    int* Ld = reinterpret_cast<int*>(dtw_lds + 3 * (size_t)Ty);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = P.n_ceps ? P.n_ceps : P.mel_dim;
    const int Lx = gt_dtw_len(P.x_len, b, Tx), Ly = gt_dtw_len(P.y_len, b, Ty);
    const double* fx = P.fx + (int64_t)b * Tx * F;
    const double* fy = P.fy + (int64_t)b * Ty * F;
    uint8_t* bp = P.path ? P.backptr + (int64_t)b * Tx * Ty : nullptr;
    const int nd = (Lx > 0 && Ly > 0) ? Lx + Ly - 1 : 0;        // anti-diagonals (uniform over the workgroup: the barriers below are too)

    for (int d = 0; d < nd; ++d) {
        const int cur = d % 3, p1 = (d + 2) % 3, p2 = (d + 1) % 3;      // the buffers of d, d - 1, d - 2
        const int j_lo = max(0, d - (Lx - 1)), j_hi = min(d, Ly - 1);
        for (int j = j_lo + ((tid - j_lo) % GT_DTW_THREADS + GT_DTW_THREADS) % GT_DTW_THREADS; j <= j_hi; j += GT_DTW_THREADS) {
            const int i = d - j;                                // 0 <= i < Lx, 0 <= j < Ly <= Ty
            const double* a = fx + i;
            const double* g = fy + j;
            double s = 0.0;
            for (int k = 0; k < F; ++k) {
                const double df = a[(int64_t)k * Tx] - g[(int64_t)k * Ty];
                s += df * df;
            }
            const double c = sqrt(s);
            double best = 0.0;
            int len = 0, dir = 0;                               // 0 diagonal, 1 up (i-1, j), 2 left (i, j-1)
            if (i > 0 && j > 0) {
                best = Dd[p2 * Ty + j - 1]; len = Ld[p2 * Ty + j - 1];
                const double up = Dd[p1 * Ty + j], left = Dd[p1 * Ty + j - 1];
                if (up < best) { best = up; len = Ld[p1 * Ty + j]; dir = 1; }
                if (left < best) { best = left; len = Ld[p1 * Ty + j - 1]; dir = 2; }
            } else if (i > 0) {
                best = Dd[p1 * Ty + j]; len = Ld[p1 * Ty + j]; dir = 1;
            } else if (j > 0) {
                best = Dd[p1 * Ty + j - 1]; len = Ld[p1 * Ty + j - 1]; dir = 2;
            }
            Dd[cur * Ty + j] = c + best;
            Ld[cur * Ty + j] = len + 1;
            if (bp) bp[(int64_t)i * Ty + j] = (uint8_t)dir;
        }
        __syncthreads();
    }

    const int last = nd ? (nd - 1) % 3 : 0;
    const int n = nd ? Ld[last * Ty + Ly - 1] : 0;              // 1 <= n <= Lx + Ly - 1 by construction
    if (tid == 0) {
        P.cost[b] = nd ? Dd[last * Ty + Ly - 1] : 0.0;
        P.path_len[b] = n;
    }
    if (!P.path) return;
    const int rows = Tx + Ty - 1;
    int32_t* path = P.path + (int64_t)b * rows * 2;
    for (int s = 2 * n + tid; s < 2 * rows; s += GT_DTW_THREADS) path[s] = -1;
    if (tid == 0) {                                             // (its own back-pointer stores are behind the sweep's last barrier)
        int i = Lx - 1, j = Ly - 1;
        for (int s = n - 1; s >= 0; --s) {
            path[2 * s] = i;
            path[2 * s + 1] = j;
            if (s == 0) break;
            const int dir = bp[(int64_t)i * Ty + j];
            if (dir != 2) --i;
            if (dir != 1) --j;
            i = max(i, 0); j = max(j, 0);                       // (never taken on a consistent table: a bound, not a rule)
        }
    }
}

size_t gt_dtw_lds_bytes(int Ty) { return (size_t)3 * Ty * (sizeof(double) + sizeof(int)); }

hipError_t gt_dtw_init() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(gt_dtw_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               GT_DTW_MAX_LDS);
}

hipError_t gt_launch_mel_dtw(const DtwArgs& a, hipStream_t stream) {
    if (!a.x || !a.y || !a.fx || !a.fy || !a.cost || !a.path_len || (a.path && !a.backptr) || (a.n_ceps && !a.basis))
        return hipErrorInvalidValue;
    if (a.B < 1 || a.Tx < 1 || a.Ty < 1 || a.mel_dim < 1 || a.n_ceps < 0 || a.n_ceps >= a.mel_dim || gt_dtw_lds_bytes(a.Ty) > GT_DTW_MAX_LDS)
        return hipErrorInvalidValue;
    const int F = a.n_ceps ? a.n_ceps : a.mel_dim;
    const int64_t n = (int64_t)a.B * ((int64_t)a.Tx + a.Ty) * F;
    const int blocks = (int)std::min<int64_t>((n + GT_DTW_FEAT_THREADS - 1) / GT_DTW_FEAT_THREADS, 1 << 16);
    hipLaunchKernelGGL(gt_dtw_features_kernel, dim3(blocks), dim3(GT_DTW_FEAT_THREADS), 0, stream, a);
    hipLaunchKernelGGL(gt_dtw_align_kernel, dim3(a.B), dim3(GT_DTW_THREADS), gt_dtw_lds_bytes(a.Ty), stream, a);
    return hipGetLastError();
}
