// Code objects: HIP loads each .hip translation unit's code object on a device
// at the first launch of one of its kernels (post.hip's, with the rocPRIM sorts,
// is 14 MB and takes ~30 ms), so sks_ctx_create launches one empty kernel per
// unit (load_code_objects, ctx.cpp) and a context's first build does not pay it.
#pragma once
#include <hip/hip_runtime.h>

namespace sks {

#define SKS_TU_LIST(X) X(abund) X(ani) X(cluster) X(downsample) X(filter) X(gather) X(ingress) X(intersect) X(join) X(layout) X(merge) X(post) X(scan) X(search) X(tally) X(topk) X(windows)
#define SKS_DECLARE_HOOK(tu) hipError_t code_object_hook_##tu(hipStream_t s);
SKS_TU_LIST(SKS_DECLARE_HOOK)
#undef SKS_DECLARE_HOOK
#define SKS_CODE_OBJECT_HOOK(tu)                                    \
  __global__ void k_code_object_##tu() {}                           \
  hipError_t code_object_hook_##tu(hipStream_t s) {                 \
    hipLaunchKernelGGL(k_code_object_##tu, dim3(1), dim3(1), 0, s); \
    return hipGetLastError();                                       \
  }

}  // namespace sks
