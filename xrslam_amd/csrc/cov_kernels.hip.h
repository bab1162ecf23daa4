// cov_kernels.hip.h -- marginal covariance of the window states and landmark depths (xrhip_ba_covariance).
//
// Runs BESIDE the solve: it reads what one linearisation leaves in HBM (Hpp, hll, Wt) and the MFMA Schur product T of
// ba_kernels.hip.h, and writes only its own scratch.  The reduced system S = Hpp - T over the na free frame dofs is Jacobi-scaled,
// A = D S D with D = diag(1 / sqrt(S_ii)), padded with an identity tail to n16 = 16 * ceil(na / 16), factored A = L L^T in place
// (kc_factor), and Sigma = D A^-1 D is read off by substitutions against unit vectors (kc_selected_inverse).  A landmark's variance
// follows from the pose part of Sigma (kc_landmark_var).
//
// A is dense row-major [n16][n16]; only the tiles on and below the diagonal are read after kc_compact.  Every loop over the
// system is strided by the launch width: no kernel here assumes na <= blockDim.
// v_mfma_f64_16x16x4_f64 operands as in ba_kernels.hip.h: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15];
// D: col = lane & 15, row = (lane >> 4) + 4 * reg.
#pragma once
#include "ba_kernels.hip.h"

namespace xrhip {

constexpr int COV_MAX_NA = 15 * 64;   // order of the largest reduced system xrhip_ba_covariance accepts
constexpr int COV_NT = 512;           // workgroup of kc_factor (8 wavefronts)

struct CovStatus {
    int status;        // 0 ok, 1 a pivot failed
    int pivot;         // index (reduced system) of the failed pivot
    double min_pivot, max_pivot;   // of the scaled factor's pivots (squares of L's diagonal), rows < na
};

// Schur weights of the covariance: the undamped 1 / hll (the solve's omega carries the trust region's mu)
__global__ __launch_bounds__(256) void kc_weights(int L, const uint8_t *__restrict__ lact, const double *__restrict__ hll,
                                                  double *__restrict__ omega) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < L) omega[l] = (lact[l] && hll[l] > 0.0) ? 1.0 / hll[l] : 0.0;
}

// entry (i, j), j <= i, of the reduced system over the free frame dofs
__device__ __forceinline__ double cov_s(const BaDims &d, const BaPtrs &p, int i, int j) {
    const int a = p.act_idx[i], b = p.act_idx[j];
    const int fa = a / 15, ka = a - 15 * fa, fb = b / 15, kb = b - 15 * fb;
    double v = p.Hpp[(size_t)a * d.n + b];
    if (d.nla && ka < 6 && kb < 6) v -= p.T[(size_t)(6 * fa + ka) * d.PF + 6 * fb + kb];
    return v;
}

// A = D S D (both triangles from the lower one: exactly symmetric), identity tail, and the scales D.  One thread per entry.
__global__ __launch_bounds__(256) void kc_compact(BaDims d, BaPtrs p, int n16, double *__restrict__ A, double *__restrict__ dsc) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n16 * n16) return;
    const int r = (int)(e / n16), c = (int)(e - (size_t)r * n16);
    const int i = max(r, c), j = min(r, c);
    if (i >= d.na) {
        A[e] = (r == c) ? 1.0 : 0.0;
        if (c == 0) dsc[r] = 1.0;
        return;
    }
    const double sii = cov_s(d, p, i, i), sjj = cov_s(d, p, j, j);
    const double di = sii > 0.0 ? 1.0 / sqrt(sii) : 1.0, dj = sjj > 0.0 ? 1.0 / sqrt(sjj) : 1.0;
    A[e] = (i == j) ? sii * (di * di) : cov_s(d, p, i, j) * (di * dj);
    if (c == 0) dsc[r] = di;   // (column 0: i == r)
}

// Blocked left-looking Cholesky of A [n16][n16] in HBM, one workgroup.  Per tile column k:
//   1. every tile (t, k), t >= k, takes its update  A_tk -= sum_{j < k} L_tj L_kj^T           (matrix cores, one wavefront per tile)
//   2. wavefront 0 factors the diagonal tile (lane r holds row r; pivots travel by shuffles), checks the pivots and inverts L_kk
//   3. the panel  L_tk = A_tk L_kk^-T, t > k                                                     (matrix cores)
// Linv [n16 / 16][256] keeps the inverted diagonal tiles for the substitutions.  A pivot <= 0 (or NaN), or <= na * 2^-52 times the
// largest pivot so far, stops the factorisation: status 1 and the pivot's index.
__global__ __launch_bounds__(COV_NT) void kc_factor(int na, int n16, double *__restrict__ A, double *__restrict__ Linv,
                                                    CovStatus *__restrict__ st) {
    __shared__ double s_inv[256];
    __shared__ int s_fail;
    const int nt = n16 / 16, nw = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 15, kk = lane >> 4;
    const size_t ld = (size_t)n16;
    double minp = 1e300, maxp = 0.0;   // wavefront 0 (uniform over its lanes)
    if (threadIdx.x == 0) s_fail = 0;
    __syncthreads();
    for (int k = 0; k < nt; ++k) {
        for (int t = k + wave; t < nt; t += nw) {
            double4_t acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = A[(size_t)(16 * t + kk + 4 * r) * ld + 16 * k + i];
            for (int j = 0; j < k; ++j)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double a = -A[(size_t)(16 * t + i) * ld + 16 * j + 4 * s + kk];
                    const double b = A[(size_t)(16 * k + i) * ld + 16 * j + 4 * s + kk];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) A[(size_t)(16 * t + kk + 4 * r) * ld + 16 * k + i] = acc[r];
        }
        __syncthreads();
        if (wave == 0) {
            double a[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = A[(size_t)(16 * k + i) * ld + 16 * k + c];   // lanes >= 16 mirror lanes 0..15
            int bad = -1;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double piv = __shfl(a[j], j);
                if (16 * k + j < na) {
                    maxp = fmax(maxp, piv);
                    if (bad < 0 && !(piv > 0.0 && piv > (double)na * 0x1p-52 * maxp)) bad = j;
                    if (bad < 0) minp = fmin(minp, piv);
                }
                const double dj = sqrt(piv);
                a[j] = a[j] / dj;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) {
                    const double lcj = __shfl(a[j], c);
                    a[c] -= a[j] * lcj;
                }
            }
            if (bad >= 0) {
                if (lane == 0) {
                    st->status = 1;
                    st->pivot = 16 * k + bad;
                    s_fail = 1;
                }
            } else {
                // column `i` of L_kk^-1 by forward substitution (L_rm comes from lane r)
                double x[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    double v = (r == i) ? 1.0 : 0.0;
#pragma unroll
                    for (int m = 0; m < r; ++m) v -= __shfl(a[m], r) * x[m];
                    x[r] = v / __shfl(a[r], r);
                }
                if (lane < 16) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) A[(size_t)(16 * k + i) * ld + 16 * k + c] = (c <= i) ? a[c] : 0.0;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        s_inv[r * 16 + i] = x[r];
                        Linv[(size_t)k * 256 + r * 16 + i] = x[r];
                    }
                }
            }
        }
        __syncthreads();
        if (s_fail) break;
        for (int t = k + 1 + wave; t < nt; t += nw) {
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double a = A[(size_t)(16 * t + i) * ld + 16 * k + 4 * s + kk];
                const double b = s_inv[i * 16 + 4 * s + kk];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) A[(size_t)(16 * t + kk + 4 * r) * ld + 16 * k + i] = acc[r];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && !s_fail) {
        st->min_pivot = minp;
        st->max_pivot = maxp;
    }
}

// Sixteen columns of A^-1 per workgroup: cols [grid][16] names them (-1: an empty slot).  B [grid][n16][16] starts as the unit
// vectors; forward (L Y = B) and back (L^T X = Y) substitution run tile row by tile row from the first tile that holds a one:
// wavefront 0 applies the inverted diagonal tile, all wavefronts push the result into the rows still open (matrix cores).
//   full == 0: the back substitution stops at that first tile, and the 15 x 15 block  D X D  of the workgroup's own rows goes to
//              out [grid][225], symmetrised (the mean of the two triangles);
//   full == 1: it runs to the top, and the columns go to Sigma [n16][n16] = out (row r, column cols[c]).
__global__ __launch_bounds__(256) void kc_selected_inverse(int na, int n16, const double *__restrict__ A, const double *__restrict__ Linv,
                                                           const double *__restrict__ dsc, const int *__restrict__ cols,
                                                           double *__restrict__ Ball, int full, double *__restrict__ out,
                                                           const CovStatus *__restrict__ st) {
    if (st->status) return;
    __shared__ int sc[16];
    const int nt = n16 / 16, nw = blockDim.x >> 6, nthr = blockDim.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 15, kk = lane >> 4;
    const size_t ld = (size_t)n16;
    double *B = Ball + (size_t)blockIdx.x * n16 * 16;
    if (threadIdx.x < 16) sc[threadIdx.x] = cols[blockIdx.x * 16 + threadIdx.x];
    __syncthreads();
    int first = n16;
    for (int c = 0; c < 16; ++c)
        if (sc[c] >= 0) first = min(first, sc[c]);
    if (first >= n16) {   // nothing to solve for: a frame that is all constant
        if (!full)
            for (int e = threadIdx.x; e < 225; e += nthr) out[(size_t)blockIdx.x * 225 + e] = 0.0;
        return;
    }
    const int t_lo = first / 16, t_stop = full ? 0 : t_lo;
    for (int e = threadIdx.x + 16 * 16 * t_stop; e < n16 * 16; e += nthr) B[e] = ((e >> 4) == sc[e & 15]) ? 1.0 : 0.0;
    __syncthreads();
    for (int t = t_lo; t < nt; ++t) {
        if (wave == 0) {   // Y_t = L_tt^-1 B_t
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Linv[(size_t)t * 256 + i * 16 + 4 * s + kk], B[(size_t)(16 * t + 4 * s + kk) * 16 + i], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) B[(size_t)(16 * t + kk + 4 * r) * 16 + i] = acc[r];
        }
        __syncthreads();
        for (int u = t + 1 + wave; u < nt; u += nw) {   // B_u -= L_ut Y_t
            double4_t acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = B[(size_t)(16 * u + kk + 4 * r) * 16 + i];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[(size_t)(16 * u + i) * ld + 16 * t + 4 * s + kk], B[(size_t)(16 * t + 4 * s + kk) * 16 + i], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) B[(size_t)(16 * u + kk + 4 * r) * 16 + i] = acc[r];
        }
        __syncthreads();
    }
    for (int t = nt - 1; t >= t_stop; --t) {
        if (wave == 0) {   // X_t = L_tt^-T B_t
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Linv[(size_t)t * 256 + (4 * s + kk) * 16 + i], B[(size_t)(16 * t + 4 * s + kk) * 16 + i], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) B[(size_t)(16 * t + kk + 4 * r) * 16 + i] = acc[r];
        }
        __syncthreads();
        for (int u = t_stop + wave; u < t; u += nw) {   // B_u -= L_tu^T X_t
            double4_t acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = B[(size_t)(16 * u + kk + 4 * r) * 16 + i];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[(size_t)(16 * t + 4 * s + kk) * ld + 16 * u + i], B[(size_t)(16 * t + 4 * s + kk) * 16 + i], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) B[(size_t)(16 * u + kk + 4 * r) * 16 + i] = acc[r];
        }
        __syncthreads();
    }
    if (full) {
        for (int e = threadIdx.x; e < na * 16; e += nthr) {
            const int r = e >> 4, c = sc[e & 15];
            if (c >= 0 && c < na) out[(size_t)r * ld + c] = B[e] * (dsc[r] * dsc[c]);
        }
    } else {
        for (int e = threadIdx.x; e < 225; e += nthr) {
            const int r = e / 15, c = e - 15 * r;
            const int ir = sc[r], ic = sc[c];
            double v = 0.0;
            if (ir >= 0 && ic >= 0) {
                const double dd = dsc[ir] * dsc[ic];
                v = (B[(size_t)ir * 16 + c] * dd + B[(size_t)ic * 16 + r] * dd) * 0.5;
            }
            out[(size_t)blockIdx.x * 225 + e] = v;
        }
    }
}

// The selected 15 x 15 blocks out of a full Sigma [n16][n16] (the landmark path), symmetrised like the blocks of the direct path.
__global__ __launch_bounds__(256) void kc_gather_blocks(int n16, const double *__restrict__ Sigma, const int *__restrict__ cols,
                                                        double *__restrict__ out, const CovStatus *__restrict__ st) {
    if (st->status) return;
    const int e = threadIdx.x;
    if (e >= 225) return;
    const int r = e / 15, c = e - 15 * r;
    const int ir = cols[blockIdx.x * 16 + r], ic = cols[blockIdx.x * 16 + c];
    double v = 0.0;
    if (ir >= 0 && ic >= 0) v = (Sigma[(size_t)ir * n16 + ic] + Sigma[(size_t)ic * n16 + ir]) * 0.5;
    out[(size_t)blockIdx.x * 225 + e] = v;
}

// var_l = 1 / hll_l + w_l^T Sigma_pp w_l / hll_l^2 with w_l the landmark's row of Wt over the free pose dofs.  One wavefront per
// four landmarks, sixteen lanes each: lane q takes the entries a = q, q + 16, ... of w_l (most are zero: a landmark is seen by a
// few frames) and their rows of Sigma.  A constant landmark gets 0.
__global__ __launch_bounds__(64) void kc_landmark_var(BaDims d, BaPtrs p, int n16, const double *__restrict__ Sigma,
                                                      double *__restrict__ var, const CovStatus *__restrict__ st) {
    if (st->status) return;
    const int lane = threadIdx.x & 63, q = lane & 15;
    const int l = blockIdx.x * 4 + (lane >> 4);
    const bool live = l < d.L && p.lact[l];
    const int P6 = 6 * d.F;
    double acc = 0.0;
    if (live) {
        const double *w = p.Wt + (size_t)l * d.PF;
        for (int a = q; a < P6; a += 16) {
            const double wa = w[a];
            if (wa == 0.0) continue;
            const int ia = p.act_inv[15 * (a / 6) + a % 6];
            if (ia < 0) continue;
            const double *row = Sigma + (size_t)ia * n16;
            double s = 0.0;
            for (int b = 0; b < P6; ++b) {
                const double wb = w[b];
                if (wb == 0.0) continue;
                const int ib = p.act_inv[15 * (b / 6) + b % 6];
                if (ib >= 0) s += row[ib] * wb;
            }
            acc += wa * s;
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (q == 0 && l < d.L) {
        const double h = live ? p.hll[l] : 0.0;
        var[l] = (live && h > 0.0) ? 1.0 / h + acc / (h * h) : 0.0;
    }
}

}   // namespace xrhip
