// Entry points that are not tied to one kernel family: versioning, error text,
// device probing.  Part of libaligner_amd.so (see include/aligner_amd.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include <mutex>
#include <cstring>
#include <map>
#include <utility>

#include "common.h"

namespace aligner {

char *error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}

unsigned long long *g_debug_stamps = nullptr;

// Development switches (aligner_debug_set_option): default from the environment, read once.
static int env_flag(const char *name) { const char *e = getenv(name); return e && e[0] && e[0] != '0'; }
#define ALIGNER_DEFINE_OPTION(name, initial, what) int g_opt_##name = initial;
ALIGNER_DEBUG_OPTIONS(ALIGNER_DEFINE_OPTION)
#undef ALIGNER_DEFINE_OPTION

hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    // the attribute is a property of (device, kernel): a grant on one device says nothing about another
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> granted;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, kernel);
    auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) granted[key] = bytes;
    return e;
}

int device_cu_count() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    static std::mutex mu;
    static std::map<int, int> counts;
    std::lock_guard<std::mutex> lock(mu);
    auto it = counts.find(dev);
    if (it != counts.end()) return it->second;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 1;
    counts[dev] = v;
    return v;
}

int device_lds_limit() {
    // gfx950 lets one workgroup own the CU's whole 160 KiB LDS; cached per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 64 * 1024;
    static std::mutex mu;
    static std::map<int, int> limits;
    std::lock_guard<std::mutex> lock(mu);
    auto it = limits.find(dev);
    if (it != limits.end()) return it->second;
    int lim = 64 * 1024, v = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
        lim = 160 * 1024;
    else if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
        lim = v;
    limits[dev] = lim;
    return lim;
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace aligner

extern "C" {

int aligner_abi_version(void) { return ALIGNER_ABI_VERSION; }

const char *aligner_last_error(void) { return aligner::error_buffer(); }

void aligner_debug_set_stamps(void *stamps_dev) {
    aligner::g_debug_stamps = static_cast<unsigned long long *>(stamps_dev);
}

int aligner_debug_set_option(const char *name, int value) {
    if (!name) return aligner::fail(ALIGNER_EINVAL, "null option name");
#define ALIGNER_SET_OPTION(opt, initial, what) \
    if (std::strcmp(name, #opt) == 0) { aligner::g_opt_##opt = value; return ALIGNER_OK; }
    ALIGNER_DEBUG_OPTIONS(ALIGNER_SET_OPTION)
#undef ALIGNER_SET_OPTION
    return aligner::fail(ALIGNER_EINVAL, "unknown option '%s'", name);
}

int aligner_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

}  // extern "C"
