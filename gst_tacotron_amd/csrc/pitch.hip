// Prosody metrics of the free run (gsttaco_pitch, gsttaco_pitch_errors: include/gsttaco.h).  Off the mel-frame hot path; double
// throughout after the fp32 load.
//
//   gt_pitch_kernel          YIN (de Cheveigne & Kawahara 2002, steps 2-5), one workgroup per frame of the mel front end's grid.  The
//                            frame's W + tau_max samples are staged in LDS once (fp32, as they are stored: a sample outside the cut
//                            signal reads 0.0).  A lane owns one lag: x[j] is a broadcast read, x[j + tau] stride-1 across the lanes, the
//                            difference function has one double accumulator per lag summed in ascending j.  The workgroup has as many
//                            waves as the lags need (up to 1024 lanes; a lane loops beyond that), so tau_max + 1 = 321 runs as six waves
//                            in one pass.  Then: lane 0 sums the running total in ascending lag, every lane divides its lags, the first
//                            lag under the threshold and the minimum are integer atomics on LDS (a minimum has no order), lane 0 walks
//                            down the dip and interpolates on the raw difference function.
//   gt_pitch_errors_kernel   one workgroup per utterance: the cells of the path (or the diagonal) strided over 256 lanes, six counts and
//                            two double sums per lane, one tree over LDS.
// Every loop is bounded by the lengths and the lag range (a NaN only ever loses a comparison), every global access by the row's clipped
// bounds, and no workgroup waits on another.  No floating-point atomics: a call is bitwise reproducible, and a row does not see its batch.
#include <algorithm>
#include <limits.h>

#include "kernels.h"
#include "device_utils.h"

#define GT_PITCH_MAX_THREADS 1024
#define GT_PERR_THREADS 256

__global__ __launch_bounds__(GT_PITCH_MAX_THREADS) void gt_pitch_kernel(PitchArgs P) {
    extern __shared__ double pitch_lds[];                       // d [tau_max + 1], running sum / d' [tau_max + 1], then the samples (fp32)
    __shared__ int s_first;
    __shared__ unsigned long long s_min;
    const int nl = P.tau_max + 1, L = P.W + P.tau_max;
    double* d = pitch_lds;
    double* c = pitch_lds + nl;
    float* xs = reinterpret_cast<float*>(pitch_lds + 2 * (size_t)nl);
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, cap = P.cap_frames;
    int start = 0, n = min(max((int)P.wav_len[b], 0), P.ld_wav);
    if (P.bounds) {                                             // (clipped again: a bound, not a rule -- the trim keeps them inside)
        start = min(max((int)P.bounds[2 * b], 0), P.ld_wav);
        n = min(max((int)P.bounds[2 * b + 1], 0), P.ld_wav - start);
    }
    const int nfr = min(n > P.n_fft / 2 ? 1 + n / P.hop : 0, cap);      // the front end's frame count (gt_trim_bounds_kernel)
    float* f0 = P.f0 + (size_t)b * cap;
    float* ap = P.aperiodicity ? P.aperiodicity + (size_t)b * cap : nullptr;
    if (t == 0 && tid == 0) P.frames[b] = nfr;
    // the grid is as wide as a row can have frames; what the caller's capacity holds beyond it is zero-filled here
    for (int64_t i = (int64_t)gridDim.x + (int64_t)t * blockDim.x + tid; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
        f0[i] = 0.f;
        if (ap) ap[i] = 0.f;
    }
    if (t >= nfr) {
        if (tid == 0) {
            f0[t] = 0.f;
            if (ap) ap[t] = 0.f;
        }
        return;
    }
    const float* x = P.wav + (size_t)b * P.ld_wav + start;
    const int u0 = t * P.hop - L / 2;
    for (int i = tid; i < L; i += blockDim.x) {
        const int u = u0 + i;
        xs[i] = (u >= 0 && u < n) ? x[u] : 0.f;
    }
    __syncthreads();
    // the difference function d(tau) = sum_{j < W} (x[j] - x[j + tau])^2; j + tau <= W - 1 + tau_max < L
    for (int tau = tid; tau < nl; tau += blockDim.x) {
        const float* xt = xs + tau;
        double acc = 0.0;
#pragma unroll 4
        for (int j = 0; j < P.W; ++j) {
            const double df = (double)xs[j] - (double)xt[j];
            acc += df * df;
        }
        d[tau] = acc;
    }
    __syncthreads();
    if (tid == 0) {                                             // the running total under d', in ascending lag
        double run = 0.0;
        c[0] = 0.0;
        for (int k = 1; k < nl; ++k) {
            run += d[k];
            c[k] = run;
        }
        s_first = INT_MAX;
        s_min = ~0ull;
    }
    __syncthreads();
    int first = INT_MAX;
    double lowest = INFINITY;
    for (int tau = tid; tau < nl; tau += blockDim.x) {
        const double sum = c[tau];
        const double dp = (tau > 0 && sum > 0.0) ? d[tau] * (double)tau / sum : 1.0;       // d'(0) = 1; d' = 1 over digital silence
        c[tau] = dp;
        if (tau >= P.tau_min) {
            if (dp < lowest) lowest = dp;
            if (tau < P.tau_max && dp < P.threshold && tau < first) first = tau;
        }
    }
    if (first != INT_MAX) atomicMin(&s_first, first);
    // d' >= 0: the bits of a non-negative double order as the values do
    if (lowest != INFINITY) atomicMin(&s_min, (unsigned long long)__double_as_longlong(lowest));
    __syncthreads();
    if (tid != 0) return;
    int tau = s_first;
    if (tau == INT_MAX) {                                       // unvoiced
        f0[t] = 0.f;
        if (ap) ap[t] = s_min == ~0ull ? 1.f : (float)__longlong_as_double((long long)s_min);
        return;
    }
    while (tau + 1 < P.tau_max && c[tau + 1] < c[tau]) ++tau;   // down the dip (2 <= tau_min <= tau < tau_max)
    const double a = d[tau - 1], m = d[tau], e = d[tau + 1];
    const double den = a - 2.0 * m + e;                         // the parabola through the RAW difference function
    const double off = den > 0.0 ? (a - e) / (2.0 * den) : 0.0;
    f0[t] = (float)(P.sr / ((double)tau + off));
    if (ap) ap[t] = (float)c[tau];
}

hipError_t gt_launch_pitch(const PitchArgs& a, hipStream_t stream) {
    if (!a.wav || !a.wav_len || !a.f0 || !a.frames) return hipErrorInvalidValue;
    if (a.B < 1 || a.ld_wav < 1 || a.cap_frames < 1 || a.hop < 1 || a.W < 1 || a.tau_min < 2 || a.tau_min >= a.tau_max ||
        a.W + a.tau_max > GT_PITCH_MAX_SPAN)
        return hipErrorInvalidValue;
    const int nl = a.tau_max + 1, L = a.W + a.tau_max;
    const int threads = std::min(GT_PITCH_MAX_THREADS, (nl + 63) / 64 * 64);
    const int gx = std::min(a.cap_frames, 1 + a.ld_wav / a.hop);
    const size_t lds = 2 * (size_t)nl * sizeof(double) + (size_t)L * sizeof(float);
    hipLaunchKernelGGL(gt_pitch_kernel, dim3(gx, a.B), dim3(threads), lds, stream, a);
    return hipGetLastError();
}

__device__ __forceinline__ int gt_perr_len(const int32_t* len, int b, int T) { return len ? min(max((int)len[b], 0), T) : T; }

__global__ __launch_bounds__(GT_PERR_THREADS) void gt_pitch_errors_kernel(PitchErrorArgs P) {
    __shared__ int sc[6][GT_PERR_THREADS];
    __shared__ double ss[2][GT_PERR_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lx = gt_perr_len(P.x_len, b, P.Tx), Ly = gt_perr_len(P.y_len, b, P.Ty);
    const float* fx = P.f0_x + (size_t)b * P.Tx;
    const float* fy = P.f0_y + (size_t)b * P.Ty;
    const int32_t* path = P.path ? P.path + (size_t)b * P.path_cap * 2 : nullptr;
    const int cells = path ? gt_perr_len(P.path_len, b, P.path_cap) : min(Lx, Ly);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    double s1 = 0.0, s2 = 0.0;
    for (int s = tid; s < cells; s += GT_PERR_THREADS) {
        const int i = path ? path[2 * s] : s, j = path ? path[2 * s + 1] : s;
        if (i < 0 || i >= Lx || j < 0 || j >= Ly) continue;     // skipped, never read
        const double x = (double)fx[i], y = (double)fy[j];
        const bool vx = x > 0.0, vy = y > 0.0;
        ++cnt[0];
        cnt[4] += vx;
        cnt[5] += vy;
        cnt[3] += vx != vy;
        if (vx && vy) {
            ++cnt[1];
            if (fabs(x - y) > P.gross * y) ++cnt[2];
            else {
                const double cents = 1200.0 * log2(x / y);
                s1 += fabs(cents);
                s2 += cents * cents;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sc[k][tid] = cnt[k];
    ss[0][tid] = s1;
    ss[1][tid] = s2;
    __syncthreads();
    for (int s = GT_PERR_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 6; ++k) sc[k][tid] += sc[k][tid + s];
            ss[0][tid] += ss[0][tid + s];
            ss[1][tid] += ss[1][tid + s];
        }
        __syncthreads();
    }
    if (tid < 6) P.counts[(size_t)b * 6 + tid] = sc[tid][0];
    if (tid < 2) P.sums[(size_t)b * 2 + tid] = ss[tid][0];
}

hipError_t gt_launch_pitch_errors(const PitchErrorArgs& a, hipStream_t stream) {
    if (!a.f0_x || !a.f0_y || !a.counts || !a.sums || (a.path && !a.path_len)) return hipErrorInvalidValue;
    if (a.B < 1 || a.Tx < 1 || a.Ty < 1 || (a.path && a.path_cap < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gt_pitch_errors_kernel, dim3(a.B), dim3(GT_PERR_THREADS), 0, stream, a);
    return hipGetLastError();
}
