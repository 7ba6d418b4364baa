// runtime.hip -- the library's runtime entry points: the ABI version and the
// thread-local error string that every other unit reports through
// (DPVO_CHECK_* in common.hpp).  Host code only.
#include "common.hpp"

namespace dpvo {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

}  // namespace dpvo

extern "C" int dpvo_hot_abi_version(void) { return DPVO_HOT_ABI_VERSION; }
extern "C" const char* dpvo_hot_last_error(void) { return dpvo::g_last_error.c_str(); }
