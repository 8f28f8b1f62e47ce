// Asynchronous single-launch Newton solve, flamingo dimensions.
#include "newton_async_impl.h"
namespace cimpc {
CIMPC_DEFINE_ASYNC_MODEL(flamingo)
}  // namespace cimpc
