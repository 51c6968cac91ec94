// probe.hip -- tsu_probe_screen: the two numbers of the heat-bath kernels' fp32 screen (disorder_dev.h) for arrays of inputs, so
// that a test can hold the device's __expf and rcp against the error bound the screen's margin rests on.  No sweep calls this
// file.  probe_tm restates the screen's four lines for x, A, t and m word for word (tests/test_screen_cpu.py compares the two
// texts); the decision rule itself, the two comparisons and the exact threshold, is written once and not here.  Built with the
// sweeps' flags, A + 4 contracts into one fused multiply-add of a32 |c32| + 4 here as it does there: the tests' twin rounds m once.
#include "tsu_common.h"

struct ScreenTM {
    float t, m;
};

__device__ __forceinline__ ScreenTM probe_tm(float f32, float a32, float c32) {
    const float x = f32 * c32;
    const float A = a32 * fabsf(c32);
    const float t = __builtin_amdgcn_rcpf(1.0f + __expf(-x)) * 65536.0f;
    const float m = (A + 4.0f) * (1.0f / 64.0f);
    return {t, m};
}

__global__ void __launch_bounds__(256) probe_screen_kernel(long long n, const float* __restrict__ f32, const float* __restrict__ a32,
                                                           const float* __restrict__ c32, float* __restrict__ t_out,
                                                           float* __restrict__ m_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ScreenTM s = probe_tm(f32[i], a32[i], c32[i]);
    t_out[i] = s.t;
    m_out[i] = s.m;
}

extern "C" int tsu_probe_screen(tsu_ctx* ctx, int64_t n, const float* f32, const float* a32, const float* c32, float* t_out,
                                float* m_out) {
    TSU_ENTER(ctx);
    if (!ctx) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, n > 0 && n <= (int64_t)1 << 31 && f32 && a32 && c32 && t_out && m_out, "tsu_probe_screen: bad arguments");
    const size_t bytes = (size_t)n * sizeof(float);
    float* d = nullptr;  // five arrays of n floats: f32, a32, c32, t, m
    TSU_HIP_TRY(ctx, hipMalloc(&d, 5 * bytes));
    const float* in[3] = {f32, a32, c32};
    float* out[2] = {t_out, m_out};
    hipError_t e = hipSuccess;
    do {
        for (int k = 0; k < 3 && e == hipSuccess; ++k)
            e = hipMemcpyAsync(d + (size_t)k * n, in[k], bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) break;
        probe_screen_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>((long long)n, d, d + (size_t)n, d + 2 * (size_t)n,
                                                                                   d + 3 * (size_t)n, d + 4 * (size_t)n);
        if ((e = hipGetLastError()) != hipSuccess) break;
        for (int k = 0; k < 2 && e == hipSuccess; ++k)
            e = hipMemcpyAsync(out[k], d + (size_t)(3 + k) * n, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) break;
        e = hipStreamSynchronize(ctx->stream);
    } while (0);
    int rc = TSU_OK;
    if (e != hipSuccess) rc = tsu_fail(ctx, TSU_E_HIP, "tsu_probe_screen: %s", hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}
