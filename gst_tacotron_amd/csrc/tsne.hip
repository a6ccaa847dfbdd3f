// The style map: exact t-SNE of style embeddings (gsttaco_style_affinities, gsttaco_style_map: include/gsttaco.h).  Off the mel-frame hot
// path; double throughout after the fp32 load.
//
//   gt_tsne_dist_kernel      squared distances, a 64 x 16 tile of the [N, N] matrix per workgroup, the rows of both sides staged in LDS
//                            32 channels at a time.  One accumulator per pair, ascending channel, the square and the sum rounded
//                            separately (contraction is switched off there), so d is the same double wherever it is computed and
//                            d_ij == d_ji bitwise.  Written into the caller's p.
//   gt_tsne_search_kernel    one workgroup per row.  A lane keeps its (up to GT_TSNE_PER_LANE) shifted distances in registers for the
//                            whole search -- N <= 1024 * 8 is the entries' cap -- and every round is one exp per entry, a fixed-order
//                            sum of the two totals (lane, wave butterfly, the waves' totals in ascending wave) and the decision, which
//                            every lane takes from the same bits.  The row of p is overwritten with p_{j|i}.
//   gt_tsne_symmetrize_kernel  p_ij = (p_{j|i} + p_{i|j}) / (2N) in place: a workgroup owns a pair of mirrored 32 x 32 tiles, reads both
//                            through LDS and writes both, so no second [N, N] buffer exists.
//   gt_tsne_pair_kernel      per descent step: a wave per row i (four rows a workgroup), the map's points tiled through LDS 1024 at a
//                            time, lane l visiting j = l, l + 64, ... in ascending j: S_i, A_i, B_i (the header's pair terms), each
//                            summed lane-wise and then over the wave's butterfly.  As <true>: the row's share of the KL divergence.
//   gt_tsne_update_kernel    one workgroup: Z in a fixed order, the update of gains, velocity and y, the column means, the recentring.
//                            Also sums Z alone (for the KL) and the rows' KL shares.
// Every loop is bounded by N and the round / step counts, every global access by N, and no workgroup waits on another.  No
// floating-point atomics: every sum has one order, so two calls are bitwise equal.
#include <algorithm>
#include <math.h>

#include "kernels.h"
#include "device_utils.h"

#define GT_TSNE_SEARCH_THREADS 1024
#define GT_TSNE_PER_LANE (GT_TSNE_MAX_N / GT_TSNE_SEARCH_THREADS)
#define GT_TSNE_ROUNDS 200
#define GT_TSNE_PAIR_THREADS 256
#define GT_TSNE_PAIR_ROWS (GT_TSNE_PAIR_THREADS / GT_WAVE)
#define GT_TSNE_Y_TILE 1024
#define GT_TSNE_UPDATE_THREADS 1024

static_assert(GT_TSNE_PER_LANE * GT_TSNE_SEARCH_THREADS == GT_TSNE_MAX_N, "the search keeps a whole row in its lanes' registers");

// over the 64 lanes, every lane holding the same bits: the xor butterfly, whose additions commute pairwise
__device__ __forceinline__ double gt_tsne_wave_sum(double s) {
#pragma unroll
    for (int d = 1; d < GT_WAVE; d <<= 1) s += __shfl_xor(s, d, GT_WAVE);
    return s;
}
__device__ __forceinline__ double gt_tsne_wave_min(double m) {
#pragma unroll
    for (int d = 1; d < GT_WAVE; d <<= 1) m = fmin(m, __shfl_xor(m, d, GT_WAVE));
    return m;
}

// ---------------------------------------------------------------------------------------------------- affinities
__global__ __launch_bounds__(256) void gt_tsne_dist_kernel(TsneAffinityArgs P) {
    __shared__ float xj[64][33];
    __shared__ float xi[16][33];
    const int tid = threadIdx.x, jl = tid & 63, ig = tid >> 6;
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * 16;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < P.D; k0 += 32) {
        for (int e = tid; e < 64 * 32; e += 256) {              // 32 consecutive channels of a row: one 128-byte line
            const int r = e >> 5, k = e & 31, j = j0 + r;
            xj[r][k] = (j < P.N && k0 + k < P.D) ? P.x[(size_t)j * P.ldx + k0 + k] : 0.f;
        }
        for (int e = tid; e < 16 * 32; e += 256) {
            const int r = e >> 5, k = e & 31, i = i0 + r;
            xi[r][k] = (i < P.N && k0 + k < P.D) ? P.x[(size_t)i * P.ldx + k0 + k] : 0.f;
        }
        __syncthreads();
        const int kn = min(32, P.D - k0);
        for (int k = 0; k < kn; ++k) {
#pragma clang fp contract(off)                                  // the square is rounded before it is added
            const double b = (double)xj[jl][k];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double df = (double)xi[ig * 4 + r][k] - b;
                const double sq = df * df;
                acc[r] = acc[r] + sq;
            }
        }
        __syncthreads();
    }
    const int j = j0 + jl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ig * 4 + r;
        if (i < P.N && j < P.N) P.p[(size_t)i * P.N + j] = acc[r];
    }
}

__global__ __launch_bounds__(GT_TSNE_SEARCH_THREADS) void gt_tsne_search_kernel(TsneAffinityArgs P) {
    __shared__ double red[2][2][GT_TSNE_SEARCH_THREADS / GT_WAVE];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (GT_WAVE - 1), wave = tid >> 6, nw = blockDim.x >> 6;
    double* row = P.p + (size_t)i * P.N;
    double dl[GT_TSNE_PER_LANE], w[GT_TSNE_PER_LANE];
    double lowest = INFINITY;
#pragma unroll
    for (int r = 0; r < GT_TSNE_PER_LANE; ++r) {
        const int j = tid + r * (int)blockDim.x;
        dl[r] = (j < P.N && j != i) ? row[j] : INFINITY;       // an entry that does not take part: exp(-beta inf) = 0
        lowest = fmin(lowest, dl[r]);
    }
    lowest = gt_tsne_wave_min(lowest);
    if (lane == 0) red[0][0][wave] = lowest;
    __syncthreads();
    for (int k = 0; k < nw; ++k) lowest = fmin(lowest, red[0][0][k]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GT_TSNE_PER_LANE; ++r) dl[r] -= lowest;
    const double target = log((double)P.perplexity);
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, s = 1.0;
    int rounds = 0;
    bool found = false;
    // one more pass than the rounds: after GT_TSNE_ROUNDS undecided rounds the weights are taken once more at the beta they left
    for (int it = 0; it <= GT_TSNE_ROUNDS && !found; ++it) {
        double ps = 0.0, pt = 0.0;
#pragma unroll
        for (int r = 0; r < GT_TSNE_PER_LANE; ++r) {
            const bool used = dl[r] != INFINITY;
            w[r] = used ? exp(-beta * dl[r]) : 0.0;
            ps += w[r];
            pt += used ? dl[r] * w[r] : 0.0;
        }
        ps = gt_tsne_wave_sum(ps);
        pt = gt_tsne_wave_sum(pt);
        if (lane == 0) {
            red[it & 1][0][wave] = ps;
            red[it & 1][1][wave] = pt;
        }
        __syncthreads();                                        // (one barrier a round: the next round writes the other half of red)
        s = 0.0;
        double t = 0.0;
        for (int k = 0; k < nw; ++k) {
            s += red[it & 1][0][k];
            t += red[it & 1][1][k];
        }
        if (it == GT_TSNE_ROUNDS) break;
        const double hd = log(s) + beta * t / s - target;
        ++rounds;
        if (fabs(hd) < 1e-5) found = true;
        else if (hd > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {                                                // (a NaN lands here: the loop stays bounded)
            hi = beta;
            beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
#pragma unroll
    for (int r = 0; r < GT_TSNE_PER_LANE; ++r) {
        const int j = tid + r * (int)blockDim.x;
        if (j < P.N) row[j] = j == i ? 0.0 : w[r] / s;
    }
    if (tid == 0) {
        P.beta[i] = beta;
        if (P.search_iters) P.search_iters[i] = rounds;
    }
}

__global__ __launch_bounds__(256) void gt_tsne_symmetrize_kernel(TsneAffinityArgs P) {
    __shared__ double ta[32][33], tb[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                                        // the mirrored pair belongs to (bj, bi)'s workgroup
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const double scale = 2.0 * (double)P.N;
    for (int r = ty; r < 32; r += 8) {
        const int ia = bi * 32 + r, ja = bj * 32 + tx, ib = bj * 32 + r, jb = bi * 32 + tx;
        ta[r][tx] = (ia < P.N && ja < P.N) ? P.p[(size_t)ia * P.N + ja] : 0.0;
        tb[r][tx] = (ib < P.N && jb < P.N) ? P.p[(size_t)ib * P.N + jb] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int ia = bi * 32 + r, ja = bj * 32 + tx, ib = bj * 32 + r, jb = bi * 32 + tx;
        // a + b and b + a are the same double: p_ij == p_ji bitwise
        if (ia < P.N && ja < P.N) P.p[(size_t)ia * P.N + ja] = ia == ja ? 0.0 : (ta[r][tx] + tb[tx][r]) / scale;
        if (bi != bj && ib < P.N && jb < P.N) P.p[(size_t)ib * P.N + jb] = (tb[r][tx] + ta[tx][r]) / scale;
    }
}

hipError_t gt_launch_style_affinities(const TsneAffinityArgs& a, hipStream_t stream) {
    if (!a.x || !a.p || !a.beta || a.N < 3 || a.N > GT_TSNE_MAX_N || a.D < 1 || a.ldx < a.D) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gt_tsne_dist_kernel, dim3((a.N + 63) / 64, (a.N + 15) / 16), dim3(256), 0, stream, a);
    const int threads = std::min(GT_TSNE_SEARCH_THREADS, (a.N + GT_WAVE - 1) / GT_WAVE * GT_WAVE);
    hipLaunchKernelGGL(gt_tsne_search_kernel, dim3(a.N), dim3(threads), 0, stream, a);
    const int tiles = (a.N + 31) / 32;
    hipLaunchKernelGGL(gt_tsne_symmetrize_kernel, dim3(tiles, tiles), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- the descent
// partials: [5][N] = S, A_x, A_y, B_x, B_y (as <true>: [0][N] = the rows' KL shares, with Z read from partials[5 N])
template <bool KL>
__global__ __launch_bounds__(GT_TSNE_PAIR_THREADS) void gt_tsne_pair_kernel(TsneMapArgs P) {
    __shared__ double ys[GT_TSNE_Y_TILE][2];
    const int tid = threadIdx.x, lane = tid & (GT_WAVE - 1), N = P.N;
    const int i = blockIdx.x * GT_TSNE_PAIR_ROWS + (tid >> 6);
    const bool live = i < N;
    const double yx = live ? P.y[2 * (size_t)i] : 0.0, yy = live ? P.y[2 * (size_t)i + 1] : 0.0;
    const double* prow = P.p + (size_t)(live ? i : 0) * N;
    const double Z = KL ? P.partials[5 * (size_t)N] : 0.0;
    double s = 0.0, ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0;
    for (int j0 = 0; j0 < N; j0 += GT_TSNE_Y_TILE) {
        const int jn = min(GT_TSNE_Y_TILE, N - j0);
        __syncthreads();
        for (int e = tid; e < 2 * jn; e += GT_TSNE_PAIR_THREADS) (&ys[0][0])[e] = P.y[2 * (size_t)j0 + e];
        __syncthreads();
        if (!live) continue;
        for (int jj = lane; jj < jn; jj += GT_WAVE) {
            const int j = j0 + jj;
            if (j == i) continue;
            const double dx = yx - ys[jj][0], dy = yy - ys[jj][1];
            const double n = 1.0 / (1.0 + (dx * dx + dy * dy));
            const double p = prow[j];
            if (KL) {
                if (p > 0.0) s += p * log(p / (n / Z));
            } else {
                s += n;
                const double pn = p * n, nn = n * n;
                ax += pn * dx;
                ay += pn * dy;
                bx += nn * dx;
                by += nn * dy;
            }
        }
    }
    s = gt_tsne_wave_sum(s);
    if (!KL) {
        ax = gt_tsne_wave_sum(ax);
        ay = gt_tsne_wave_sum(ay);
        bx = gt_tsne_wave_sum(bx);
        by = gt_tsne_wave_sum(by);
    }
    if (live && lane == 0) {
        P.partials[i] = s;
        if (!KL) {
            P.partials[(size_t)N + i] = ax;
            P.partials[2 * (size_t)N + i] = ay;
            P.partials[3 * (size_t)N + i] = bx;
            P.partials[4 * (size_t)N + i] = by;
        }
    }
}

// the sum of v over the workgroup, in every thread: wave butterfly, then the waves' totals in ascending wave.  Two barriers.
__device__ __forceinline__ double gt_tsne_block_sum(double v, double* red) {
    const int lane = threadIdx.x & (GT_WAVE - 1), wave = threadIdx.x >> 6;
    v = gt_tsne_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < GT_TSNE_UPDATE_THREADS / GT_WAVE; ++k) t += red[k];
    return t;
}

#define GT_TSNE_MODE_STEP 0     // Z, the update, the recentring
#define GT_TSNE_MODE_Z 1        // Z alone, into partials[5 N]
#define GT_TSNE_MODE_KL 2       // the sum of the rows' KL shares, into kl

__global__ __launch_bounds__(GT_TSNE_UPDATE_THREADS) void gt_tsne_update_kernel(TsneMapArgs P, int mode, double e, double m) {
    __shared__ double red[GT_TSNE_UPDATE_THREADS / GT_WAVE];
    const int tid = threadIdx.x, N = P.N;
    double part = 0.0;
    for (int i = tid; i < N; i += GT_TSNE_UPDATE_THREADS) part += P.partials[i];
    const double Z = gt_tsne_block_sum(part, red);              // (mode KL: the divergence)
    if (mode != GT_TSNE_MODE_STEP) {
        if (tid == 0) (mode == GT_TSNE_MODE_Z ? P.partials + 5 * (size_t)N : P.kl)[0] = Z;
        return;
    }
    double sx = 0.0, sy = 0.0;
    for (int i = tid; i < N; i += GT_TSNE_UPDATE_THREADS) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t o = 2 * (size_t)i + c;
            const double g = e * P.partials[(size_t)(1 + c) * N + i] - P.partials[(size_t)(3 + c) * N + i] / Z;
            double v = P.velocity[o], gain = P.gains[o];
            const int sg = (g > 0.0) - (g < 0.0), sv = (v > 0.0) - (v < 0.0);
            gain = sg != sv ? gain + 0.2 : gain * 0.8;
            gain = fmax(gain, 0.01);
            v = m * v - P.eta * gain * g;
            const double y = P.y[o] + v;
            P.gains[o] = gain;
            P.velocity[o] = v;
            P.y[o] = y;
            (c ? sy : sx) += y;
        }
    }
    const double mx = gt_tsne_block_sum(sx, red) / (double)N, my = gt_tsne_block_sum(sy, red) / (double)N;
    for (int i = tid; i < N; i += GT_TSNE_UPDATE_THREADS) {     // (a thread reads back what it wrote itself)
        P.y[2 * (size_t)i] -= mx;
        P.y[2 * (size_t)i + 1] -= my;
    }
}

hipError_t gt_launch_style_map(const TsneMapArgs& a, hipStream_t stream) {
    if (!a.p || !a.y || !a.velocity || !a.gains || !a.partials || a.N < 3 || a.N > GT_TSNE_MAX_N || a.iters < 0 || a.first_iter < 0)
        return hipErrorInvalidValue;
    const dim3 grid((a.N + GT_TSNE_PAIR_ROWS - 1) / GT_TSNE_PAIR_ROWS);
    for (int64_t t = a.first_iter; t < (int64_t)a.first_iter + a.iters; ++t) {
        hipLaunchKernelGGL(gt_tsne_pair_kernel<false>, grid, dim3(GT_TSNE_PAIR_THREADS), 0, stream, a);
        hipLaunchKernelGGL(gt_tsne_update_kernel, dim3(1), dim3(GT_TSNE_UPDATE_THREADS), 0, stream, a, GT_TSNE_MODE_STEP,
                           t < a.stop_lying_iter ? a.exaggeration : 1.0, t < a.mom_switch_iter ? a.momentum : a.final_momentum);
    }
    if (a.kl) {
        hipLaunchKernelGGL(gt_tsne_pair_kernel<false>, grid, dim3(GT_TSNE_PAIR_THREADS), 0, stream, a);
        hipLaunchKernelGGL(gt_tsne_update_kernel, dim3(1), dim3(GT_TSNE_UPDATE_THREADS), 0, stream, a, GT_TSNE_MODE_Z, 1.0, 0.0);
        hipLaunchKernelGGL(gt_tsne_pair_kernel<true>, grid, dim3(GT_TSNE_PAIR_THREADS), 0, stream, a);
        hipLaunchKernelGGL(gt_tsne_update_kernel, dim3(1), dim3(GT_TSNE_UPDATE_THREADS), 0, stream, a, GT_TSNE_MODE_KL, 1.0, 0.0);
    }
    return hipGetLastError();
}
