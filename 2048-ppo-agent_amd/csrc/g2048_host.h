// Host-side helpers of the C ABI entry points (include/g2048.h): the error-code contract and the pointer-alignment test.
#ifndef G2048_HOST_H
#define G2048_HOST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g2048_host {

// ABI error contract: a HIP runtime error e is reported as -(1000 + e)
inline int hip_error_code() { return -(1000 + (int)hipGetLastError()); }  // after a runtime call that has just failed
// status of the launches an entry point has just made: 0 or the error code
inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(1000 + (int)e);
}
// The dynamic-LDS limit is a per-device attribute of the kernel an entry point is about to launch: set on every call (no latch, the
// library keeps no global state).  0 or the error code.
inline int allow_dynamic_lds(const void *kernel, int bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 0 : hip_error_code();
}
// every pointer is 16-byte aligned (a null pointer counts as aligned: optional operands are tested for presence separately)
template <class... P>
inline bool aligned16(const P *...p) {
    return !((... | (uintptr_t)p) & 15);
}

}  // namespace g2048_host
#endif  // G2048_HOST_H
