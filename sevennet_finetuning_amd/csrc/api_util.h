// Error plumbing shared by the translation units behind the C ABI of
// include/e3gnn.h (api.cpp, model_load.cpp, api_train.cpp, api_nlist.cpp,
// api_d3.cpp, api_data.cpp): one thread-local last-error string for the whole library
// (defined in api.cpp, read by e3gnn_last_error).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/e3gnn.h"

namespace e3gnn {

// records `msg` as the calling thread's last error and returns `code`
int fail(int code, const std::string& msg);

// E3GNN_TRACE_ERRORS=1: report where HIP's thread-local error state got set
void trace_point(const char* where);

}  // namespace e3gnn

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return ::e3gnn::fail(E3GNN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
