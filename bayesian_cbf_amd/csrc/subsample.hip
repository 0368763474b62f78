// Random max_train subset of every instance's observation pool, selected and gathered in one launch (bcbf_subsample_rows).
//
// The reference's LearnedShiftInvariantDynamics.fit (unicycle_move_to_pose.py:377-384) shuffles the indices of the whole
// visited buffer and keeps the first max_train.  Here the caller supplies one uniform key per pool row (torch.rand: the library
// draws no random numbers); sorting the keys gives a uniformly random permutation and its first N entries are that subset, in
// shuffled order.  Output row j of instance b is the pool row with the j-th smallest key, equal keys to the lower pool index
// first -- torch.sort(keys[:, :P], stable=True).indices[:, :N] + lo exactly.
//
// One workgroup per instance: the P keys become 64-bit words (order-preserving bits of the key << 32 | pool index, so ties break
// by index), padded with UINT64_MAX to a power of two and sorted by a bitonic network in LDS (P <= 8192: 64 KB); then the
// workgroup copies the N chosen rows of X / UH / Y into the contiguous [B, N, .] layout bcbf_refit / bcbf_potrs read.  The
// writes are coalesced; the reads are scattered over one instance's stream, which is a few tens of KB.
#include "bcbf_common.h"
#include <stdio.h>

namespace bcbf {

constexpr int SS_THREADS = 256;
constexpr int SS_MAX_POOL = 8192;

// float -> uint32 with the same order as the floats (torch.sort's: -0 == +0, every NaN equal and last)
__device__ inline uint32_t ss_key_bits(float k) {
    const uint32_t u = k != k ? 0x7fc00000u : k == 0.0f ? 0u : __float_as_uint(k);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename T>
__device__ inline void ss_gather(const T* __restrict__ src, T* __restrict__ dst, const uint64_t* w, int lo, int P, int N, int d,
                                 size_t src_inst, size_t dst_inst) {
    for (int e = threadIdx.x; e < N * d; e += SS_THREADS) {
        const int j = e / d, c = e - j * d;
        const uint32_t i = (uint32_t)w[j];          // (< P by construction; the guard keeps a broken sort inside the pool)
        const int row = lo + (int)(i < (uint32_t)P ? i : 0u);
        dst[dst_inst + e] = src[src_inst + (size_t)row * d + c];
    }
}

template <typename T>
__global__ void __launch_bounds__(SS_THREADS)
subsample_rows_kernel(const float* __restrict__ keys, int ldk, int lo, int P, int Pp, const T* __restrict__ X, const T* __restrict__ UH,
                      const T* __restrict__ Y, int Ntot, int n, int C, int N, T* __restrict__ Xo, T* __restrict__ UHo,
                      T* __restrict__ Yo, int32_t* __restrict__ idx_out) {
    extern __shared__ __attribute__((aligned(16))) uint64_t ss_words[];
    const int b = blockIdx.x;
    const float* kb = keys + (size_t)b * ldk;
    for (int i = threadIdx.x; i < Pp; i += SS_THREADS)
        ss_words[i] = i < P ? ((uint64_t)ss_key_bits(kb[i]) << 32) | (uint32_t)i : ~(uint64_t)0;
    __syncthreads();
    // bitonic network over Pp words: for each (k, j) stage every thread compares-and-exchanges pairs (i, i + j), ascending where
    // bit k of i is clear.  The padding words are larger than every real word (the index field of a real word is < 8192), so
    // the first N <= P words after the sort are real rows.
    for (int k = 2; k <= Pp; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (Pp >> 1); t += SS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint64_t a = ss_words[i], c = ss_words[i + j];
                if ((a > c) == ((i & k) == 0)) { ss_words[i] = c; ss_words[i + j] = a; }
            }
            __syncthreads();
        }
    }
    const size_t sb = (size_t)b * Ntot;
    for (int j = threadIdx.x; j < N; j += SS_THREADS) {
        const uint32_t i = (uint32_t)ss_words[j];
        idx_out[(size_t)b * N + j] = lo + (int)(i < (uint32_t)P ? i : 0u);
    }
    ss_gather(X, Xo, ss_words, lo, P, N, n, sb * n, (size_t)b * N * n);
    ss_gather(UH, UHo, ss_words, lo, P, N, C, sb * C, (size_t)b * N * C);
    ss_gather(Y, Yo, ss_words, lo, P, N, n, sb * n, (size_t)b * N * n);
}

static int subsample_args_ok(const void* keys, int ldk, int lo, int P, const void* X, const void* UH, const void* Y, int Ntot, int n,
                             int m, int N, const void* Xo, const void* UHo, const void* Yo, const void* idx_out, int B) {
    static thread_local char msg[200];
    const char* why = nullptr;
    if (!keys || !X || !UH || !Y || !Xo || !UHo || !Yo || !idx_out) why = "null pointer";
    else if (B < 1) why = "B < 1";
    else if (N < 1 || N > P) why = "need 1 <= N <= P";
    else if (P > SS_MAX_POOL) why = "P > 8192 (the pool is sorted in LDS)";
    else if (lo < 0 || (long long)lo + P > Ntot) why = "need 0 <= lo and lo + P <= Ntot";
    else if (ldk < P) why = "ldk < P";
    else if (n < 1 || n > BCBF_MAX_STATE_DIM) why = "need 1 <= n <= 8";
    else if (m < 0 || m > 8) why = "need 0 <= m <= 8";
    if (!why) return 1;
    snprintf(msg, sizeof(msg), "bcbf_subsample_rows: %s (B=%d N=%d P=%d lo=%d Ntot=%d ldk=%d n=%d m=%d)", why, B, N, P, lo, Ntot, ldk, n, m);
    set_error_message(msg);
    return 0;
}

template <typename T>
static int launch_subsample_rows(const float* keys, int ldk, int lo, int P, const T* X, const T* UH, const T* Y, int Ntot, int n, int m,
                                 int N, T* Xo, T* UHo, T* Yo, int32_t* idx_out, int B, void* stream) {
    if (!subsample_args_ok(keys, ldk, lo, P, X, UH, Y, Ntot, n, m, N, Xo, UHo, Yo, idx_out, B)) return BCBF_EINVAL;
    int Pp = 2;
    while (Pp < P) Pp <<= 1;
    const size_t lds = (size_t)Pp * sizeof(uint64_t);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)subsample_rows_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(subsample_rows_kernel<T>, dim3(B), dim3(SS_THREADS), lds, (hipStream_t)stream, keys, ldk, lo, P, Pp, X, UH, Y,
                       Ntot, n, m + 1, N, Xo, UHo, Yo, idx_out);
    return check_launch("bcbf_subsample_rows");
}

}  // namespace bcbf

extern "C" int bcbf_subsample_rows_f32(const float* keys, int ldk, int lo, int P, const float* X, const float* UH, const float* Y, int Ntot,
                                       int n, int m, int N, float* Xo, float* UHo, float* Yo, int32_t* idx_out, int B, void* stream) {
    return bcbf::launch_subsample_rows(keys, ldk, lo, P, X, UH, Y, Ntot, n, m, N, Xo, UHo, Yo, idx_out, B, stream);
}
extern "C" int bcbf_subsample_rows_f64(const float* keys, int ldk, int lo, int P, const double* X, const double* UH, const double* Y,
                                       int Ntot, int n, int m, int N, double* Xo, double* UHo, double* Yo, int32_t* idx_out, int B,
                                       void* stream) {
    return bcbf::launch_subsample_rows(keys, ldk, lo, P, X, UH, Y, Ntot, n, m, N, Xo, UHo, Yo, idx_out, B, stream);
}
