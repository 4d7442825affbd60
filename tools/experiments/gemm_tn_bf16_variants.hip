// gemm_tn_bf16_variants.hip — EXPERIMENT (not product code): the buffering choice of csrc/gemm_bf16.hip's two-operand 128 x 256 tile,
// timed on the recurrent update's c3 shape (dG [131072][512]^T [xe | h] [131072][128 + 128], 128 splits of 1024 rows).
//   NBUF = 1  one slab buffer (80 640 bytes of LDS), two workgroups per CU — what the library builds
//   NBUF = 2  two slab buffers (161 280 bytes), one barrier per slab, one workgroup per CU
// The kernel is the library's own text (included with PFA_GEMM_BF16_KERNEL_ONLY); the two alternate inside one process.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature -Xclang -packed-fp32-ops -Ipufferlib_amd/csrc \
//         tools/experiments/gemm_tn_bf16_variants.hip -o tools/experiments/_bin/gemm_tn_bf16_variants
// RESULT (MI355X, profiles/r08_gemm_tn_bf16_ab.json): NBUF = 1 200.3 us per launch (min 199.6, max 210.6 over 5 rounds of 20), NBUF = 2
// 269.5 (264.8 .. 270.1), partials bit-identical: the double buffer LOST by a third — with one wave per SIMD nothing issues MFMAs while
// a workgroup splits and stores its next slab — and is not built into the library.
// Also tried at compile time only: all four A fragments of a wave resident beside the 128 accumulators (GemmBfCfg::MA = MI) needs 269+
// registers — 13 to 77 dwords spilled under the 256 of two waves per SIMD — so the library keeps two resident and reads B twice.
#define PFA_GEMM_BF16_KERNEL_ONLY
#include "../../pufferlib_amd/csrc/gemm_bf16.hip"

#include <algorithm>
#include <vector>

using namespace pfa;

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            return 3;                                                          \
        }                                                                      \
    } while (0)

__global__ void fill_kernel(float *x, size_t n, uint32_t seed) {   // uniform in [-1, 1): timing data, every bf16 piece populated
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u + seed;
        h ^= h >> 15, h *= 2246822519u, h ^= h >> 13;
        x[i] = (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
    }
}

template <int NBUF>
static int launch(const float *a, const float *b0, const float *b1, int mo, long long k, long long per, int splits, float *partial) {
    using Cfg = GemmBfCfg<2, 2, 4, 8, NBUF>;
    CK(hipFuncSetAttribute((const void *)gemm_tn_partial_bf16_kernel<2, 2, 4, 8, NBUF>, hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kBytes));
    hipLaunchKernelGGL((gemm_tn_partial_bf16_kernel<2, 2, 4, 8, NBUF>), dim3(mo / 128, splits), dim3(kGemmBfThreads), Cfg::kBytes, 0, a, (long long)mo, b0,
                       128LL, mo, 256, k, per, partial, b1, 128LL, 128);
    return 0;
}

int main() {
    const int mo = 512, splits = 128, reps = 20, rounds = 5;
    const long long k = 131072, per = k / splits;
    float *a, *b0, *b1, *p1, *p2;
    CK(hipMalloc(&a, k * mo * 4));
    CK(hipMalloc(&b0, k * 128 * 4));
    CK(hipMalloc(&b1, k * 128 * 4));
    CK(hipMalloc(&p1, (size_t)splits * mo * 256 * 4));
    CK(hipMalloc(&p2, (size_t)splits * mo * 256 * 4));
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, a, (size_t)k * mo, 1u);
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, b0, (size_t)k * 128, 2u);
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, b1, (size_t)k * 128, 3u);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> t[2];
    for (int r = 0; r <= rounds; ++r)          // round 0 warms up
        for (int v = 0; v < 2; ++v) {
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < reps; ++i)
                if (v == 0 ? launch<1>(a, b0, b1, mo, k, per, splits, p1) : launch<2>(a, b0, b1, mo, k, per, splits, p2)) return 1;
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) t[v].push_back(ms * 1e3f / reps);
        }
    std::vector<float> h1((size_t)splits * mo * 256), h2(h1.size());
    CK(hipMemcpy(h1.data(), p1, h1.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h2.data(), p2, h2.size() * 4, hipMemcpyDeviceToHost));
    const bool same = std::equal(h1.begin(), h1.end(), h2.begin());
    for (int v = 0; v < 2; ++v) {
        std::sort(t[v].begin(), t[v].end());
        printf("NBUF = %d: median %.1f us per launch (min %.1f, max %.1f over %d rounds of %d)\n", v + 1, t[v][rounds / 2], t[v].front(), t[v].back(), rounds,
               reps);
    }
    printf("partials bit-identical between the two: %s\n", same ? "yes" : "NO");
    return same ? 0 : 1;
}
