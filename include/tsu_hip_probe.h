/* tsu_hip_probe.h -- a probe of the fp32 screen of the heat-bath kernels K7 / K8 (csrc/disorder_dev.h, entry point in
 * csrc/probe.hip).  No sweep calls it: it exists so that a test can measure, on the device, the two numbers the screen compares.
 *
 * Part of the C ABI of libtsu_hip.so: included by tsu_hip.h after tsu_hip_sparse_batch.h (inside its extern "C" block); include
 * tsu_hip.h, not this file.  Its ctypes prototypes are tsu._hip.PROBE_SIGNATURES, one to one.
 */
#ifndef TSU_HIP_PROBE_H
#define TSU_HIP_PROBE_H
#ifndef TSU_HIP_H
#error "include tsu_hip.h, which includes this header"
#endif

/* For i < n: t_out[i], m_out[i] = the screen's t = 2^16 rcp(1 + __expf(-x)) and margin m = (A + 4) / 64 of the fp32 field f32[i],
 * the fp32 sum of |terms| a32[i] and the scale c32[i] = fl32(2 / T), x = f32 c32, A = a32 |c32|: the four lines of the sweeps'
 * screen restated, evaluated once per element by a flat grid.  Any fp32 value is allowed, non-finite ones included.  Host arrays
 * in and out; n <= 0 or a NULL pointer: TSU_E_INVALID.  Synchronises.  DESIGN.md, "What pins the screen". */
int tsu_probe_screen(tsu_ctx* ctx, int64_t n, const float* f32, const float* a32, const float* c32, float* t_out, float* m_out);

#endif /* TSU_HIP_PROBE_H */
