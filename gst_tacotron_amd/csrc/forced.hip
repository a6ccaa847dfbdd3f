// Teacher-forced decoding (the training=True half of the reference's decoder loop, Taco2.py:161,183-187: step t consumes the
// ground-truth frame mels[:, 0:-1:r][:, t] instead of decodings[:, -1]) needs two small kernels beside the decode step's own:
//
//   gt_stage_teacher_kernel    the consumed frames teacher[b, t*r, :] gathered step-major into w_teach [S][B][mel]: the input copy of
//                              a forced call.  Step t's frame block is then one dense [B, mel] matrix (the four-kernel front end reads it
//                              as its prenet-0 operand) and all S blocks together are the [S*B, mel] operand of ONE GEMM that computes
//                              every step's prenet-0 pre-activations up front (gsttaco.cpp enqueue_forced_z0).
//   gt_forced_durations_kernel per-token frame counts of a forced alignment: frame f of utterance b belongs to token
//                              argmax_{j < n} align[b, f / r, j], the lowest index on a tie.
#include "kernels.h"

__global__ __launch_bounds__(256) void gt_stage_teacher_kernel(const float* __restrict__ teacher, float* __restrict__ out, int B, int Tq, int S,
                                                               int r, int mel) {
    const int64_t n = (int64_t)S * B * mel;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % mel);
        const int64_t row = i / mel;            // = t * B + b
        const int b = (int)(row % B), t = (int)(row / B);
        // (t <= S - 1 and (S - 1) * r <= Tq - 2: the frame exists)
        out[i] = teacher[((int64_t)b * Tq + (int64_t)t * r) * mel + c];
    }
}

hipError_t gt_launch_stage_teacher(const float* teacher, float* out, int B, int Tq, int S, int r, int mel, hipStream_t stream) {
    if (B < 1 || S < 1 || r < 1 || mel < 1 || (int64_t)(S - 1) * r > (int64_t)Tq - 1) return hipErrorInvalidValue;
    const int64_t n = (int64_t)S * B * mel;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(gt_stage_teacher_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, teacher, out, B, Tq, S, r, mel);
    return hipGetLastError();
}

// One workgroup per utterance, one wave per decoder step at a time.  A lane scans columns lane, lane + 64, ... and keeps its first
// maximum (strict >), the wave then keeps the larger value and, between equal values, the lower index: numpy.argmax's choice.
// The step's r frames that lie below the utterance's length L are added to the winner's count (global atomics on the row this
// workgroup zeroed itself: __syncthreads orders the two within the workgroup).
__global__ __launch_bounds__(256) void gt_forced_durations_kernel(const float* __restrict__ align, const int32_t* __restrict__ tok_len,
                                                                  const int32_t* __restrict__ mel_len, int32_t* __restrict__ dur, int S, int Tv,
                                                                  int r) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* row = dur + (int64_t)b * Tv;
    for (int j = tid; j < Tv; j += 256) row[j] = 0;
    __syncthreads();
    int n = Tv;
    if (tok_len) n = max(1, min(Tv, (int)tok_len[b]));
    int64_t L = (int64_t)S * r;
    if (mel_len) L = max((int64_t)0, min(L, (int64_t)mel_len[b]));
    for (int s = wave; s < S; s += 4) {
        const int64_t f0 = (int64_t)s * r;
        if (f0 >= L) break;                     // (wave-uniform: later steps of this wave lie beyond the length as well)
        const float* a = align + ((int64_t)b * S + s) * Tv;
        float best = -INFINITY;
        int idx = n;                            // (n: nothing seen yet -- loses every tie)
        for (int j = lane; j < n; j += 64) {
            const float v = a[j];
            if (idx == n || v > best) { best = v; idx = j; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(idx, off, 64);
            if (oi < n && (idx >= n || ov > best || (ov == best && oi < idx))) { best = ov; idx = oi; }
        }
        if (lane == 0 && idx < n) atomicAdd(row + idx, (int32_t)min((int64_t)r, L - f0));
    }
}

hipError_t gt_launch_forced_durations(const float* align, const int32_t* tok_len, const int32_t* mel_len, int32_t* dur, int B, int S,
                                      int Tv, int r, hipStream_t stream) {
    if (B < 1 || S < 1 || Tv < 1 || r < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gt_forced_durations_kernel, dim3(B), dim3(256), 0, stream, align, tok_len, mel_len, dur, S, Tv, r);
    return hipGetLastError();
}
