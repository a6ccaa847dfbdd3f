// Band-limited sinc resampling of reference audio (gsttaco_resample, include/gsttaco.h): resampy's 'kaiser_best' as librosa.core.load
// applies it, ahead of the wav -> mel front end.  Off the mel-frame hot path; double throughout after the fp32 load, one rounding to
// float32 at the end.
//
//   gt_resample_kernel   one launch for a batch of rows, grid (blocks of GT_RS_THREADS outputs, rows), one thread per output sample t:
//                        reads its rate pair's accumulated time register time[t] (a double, built on the host by sequential additions:
//                        resampy accumulates it, and the truncated table step makes the interpolation discontinuous where it crosses an
//                        integer), takes n, frac, offset and eta of each wing in double exactly as the host code does, and sums
//                        (win[i] + eta * delta[i]) * x[src] in double in ONE fixed order -- left wing tap 0 upward, then right wing tap 0
//                        upward.  A row's result therefore does not depend on the batch it runs in.  The workgroup's input window
//                        [n(first t) - W + 1, n(last t) + W] (W = taps of a wing) is staged in LDS as floats; the gained table and its
//                        differences lie interleaved {win, delta} in global memory (512 KiB per rate pair, L2-resident).  Within a
//                        workgroup the outputs are dealt to the lanes in the order of their table offset (a counting sort in LDS), so
//                        a wavefront's table reads of one tap fall in a few cache lines instead of one per lane.  A row at the
//                        target rate is copied through; every row is zero-filled from its n_out to ld_out.
// Per-row parameters travel BY VALUE in the kernel arguments: a call that follows another on the stream cannot overwrite what the
// first one still reads.  Contraction is off in this file, so the sum is the mul-then-add sequence of the float64 restatement the
// tests compare with.  Every table index is below nwin by the tap count, every source index inside [0, n_in) by the tap count and
// the clamp of n, and no workgroup waits on another.
#pragma clang fp contract(off)

#include "kernels.h"
#include "device_utils.h"

// the staged window at the largest supported down-sampling factor: 255 * 16 + 2 source samples under the workgroup's outputs plus
// 2 * ceil(32769 / 32) = 2050 for the wings
#define GT_RS_LDS_FLOATS (GT_RS_THREADS * GT_RS_MAX_FACTOR + 2 * ((GT_RS_NWIN + 512 / GT_RS_MAX_FACTOR - 1) / (512 / GT_RS_MAX_FACTOR)) + 8)

__global__ __launch_bounds__(GT_RS_THREADS) void gt_resample_kernel(ResampleArgs P) {
    __shared__ float xs[GT_RS_LDS_FLOATS];
    __shared__ int bins[2 * GT_RS_THREADS], perm[GT_RS_THREADS], wave_sum[GT_RS_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int t0 = blockIdx.x * GT_RS_THREADS, t = t0 + tid;
    const int n_in = P.n_in[b], n_out = P.n_out[b], slot = P.slot[b];
    const float* x = P.x + (int64_t)(P.row0 + b) * P.ld_in;
    float* y = P.y + (int64_t)(P.row0 + b) * P.ld_out;
    if (slot == GT_RS_PASS) {                                   // already at the target rate: the samples themselves (n_out == n_in)
        if (t < P.ld_out) y[t] = t < n_out ? x[t] : 0.f;
        return;
    }
    if (t0 >= n_out) {                                          // (uniform over the workgroup)
        if (t < P.ld_out) y[t] = 0.f;
        return;
    }
    const ResamplePair pr = P.pair[slot];
    const int step = pr.step, wing = (GT_RS_NWIN + step - 1) / step;
    const int t_last = min(t0 + GT_RS_THREADS, n_out) - 1;
    // the register grows with t, so the first and last output bound every n of the workgroup
    const int n_first = min((int)pr.time[t0], n_in - 1), n_last = min((int)pr.time[t_last], n_in - 1);
    // at most 255 * 16 + 1 + 2 * 1025 samples: the launcher admits no step below 32 and no time increment above 16, so the window fits
    // (the min is a bound for the LDS writes, not a rule)
    const int lo = max(n_first - wing + 1, 0), hi = min(min(n_last + wing, n_in - 1), lo + GT_RS_LDS_FLOATS - 1);
    for (int i = tid; i <= hi - lo; i += GT_RS_THREADS) xs[i] = x[lo + i];
    __syncthreads();
    if (t < P.ld_out && t >= n_out) y[t] = 0.f;

    // Which lane computes which output is free (an output's sum does not depend on it), and the table reads want the lanes of a
    // wavefront close together: their left-wing offsets lie anywhere in a step-wide band of the table (up to 8 KiB), and one gather
    // then touches as many cache lines as it has lanes.  So the workgroup's outputs are counting-sorted by that offset (512 bins;
    // the right wing's offset is step-exact minus the left's: sorted too), and lane r takes the output of rank r.
    const double scale = pr.scale;
    const int lane = tid & 63, wave = tid >> 6;
    const bool valid = t < n_out;
    int key = 0;
    if (valid) {
        const double tm = pr.time[t];
        key = min((int)(scale * (tm - (double)min((int)tm, n_in - 1)) * 512.0), 511);
    }
    bins[tid] = 0; bins[tid + GT_RS_THREADS] = 0;
    __syncthreads();
    if (valid) atomicAdd(&bins[key], 1);
    __syncthreads();
    const int c0 = bins[2 * tid], c1 = bins[2 * tid + 1];
    int incl = c0 + c1;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int excl = incl - (c0 + c1);
    for (int w = 0; w < wave; ++w) excl += wave_sum[w];
    bins[2 * tid] = excl; bins[2 * tid + 1] = excl + c0;        // each bin's first rank, then its cursor
    __syncthreads();
    if (valid) perm[atomicAdd(&bins[key], 1)] = tid;            // (the order inside a bin is arbitrary: it decides lanes, not results)
    __syncthreads();
    if (tid > t_last - t0) return;                              // ranks 0 .. t_last - t0 are the workgroup's computed outputs
    const int tt = t0 + perm[tid];

    const double time = pr.time[tt];
    const int n = min((int)time, n_in - 1);
    double frac = scale * (time - (double)n);
    double acc = 0.0;
    for (int w = 0; w < 2; ++w) {                               // 0: left wing, x[n - i]; 1: right wing, x[n + i + 1]
        if (w) frac = scale - frac;
        const double index_frac = frac * 512.0;
        const int offset = (int)index_frac;
        const double eta = index_frac - (double)offset;
        const int count = min(w ? n_in - n - 1 : n + 1, (GT_RS_NWIN - offset) / step);
        const double2* tab = pr.table + offset;
        const int src0 = (w ? n + 1 : n) - lo, dir = w ? 1 : -1;
        for (int i = 0; i < count; ++i) {
            const double2 wd = tab[(int64_t)i * step];
            const double weight = wd.x + eta * wd.y;
            acc = acc + weight * (double)xs[src0 + dir * i];
        }
    }
    y[tt] = (float)acc;
}

hipError_t gt_launch_resample(const ResampleArgs& a, hipStream_t stream) {
    if (!a.x || !a.y || a.rows < 1 || a.rows > GT_RS_MAX_ROWS || a.row0 < 0 || a.ld_in < 1 || a.ld_out < 1) return hipErrorInvalidValue;
    for (int b = 0; b < a.rows; ++b) {
        const int slot = a.slot[b];
        if (a.n_in[b] < 0 || a.n_in[b] > a.ld_in || a.n_out[b] < 0 || a.n_out[b] > a.ld_out) return hipErrorInvalidValue;
        if (slot == GT_RS_PASS) {
            if (a.n_out[b] != a.n_in[b]) return hipErrorInvalidValue;
            continue;
        }
        if (slot >= GT_RS_MAX_PAIRS) return hipErrorInvalidValue;
        const ResamplePair& p = a.pair[slot];
        if (!p.time || !p.table || p.step < 512 / GT_RS_MAX_FACTOR || p.step > 512 || !(p.scale * GT_RS_MAX_FACTOR >= 1.0) || p.scale > 1.0 || a.n_out[b] > p.time_len)
            return hipErrorInvalidValue;
        if (a.n_out[b] > 0 && a.n_in[b] < 1) return hipErrorInvalidValue;
    }
    const dim3 grid((a.ld_out + GT_RS_THREADS - 1) / GT_RS_THREADS, a.rows);
    hipLaunchKernelGGL(gt_resample_kernel, grid, dim3(GT_RS_THREADS), 0, stream, a);
    return hipGetLastError();
}
