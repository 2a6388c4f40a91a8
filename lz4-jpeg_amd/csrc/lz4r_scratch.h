// lz4r_scratch.h -- per-call device scratch of the decoders' host sides: a
// stream-ordered allocation from a pool of the library's own per device that
// keeps its memory (lz4r_gpudec.hip has the pool); free with hipFreeAsync.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

__attribute__((visibility("hidden"))) hipError_t lz4r_scratch_alloc(void **ptr, size_t bytes,
                                                                    hipStream_t s);
