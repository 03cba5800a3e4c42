// ep24 - error plumbing of the C ABI.
#include "common.h"

static thread_local char g_err[512] = "";

void ep24_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* ep24_last_error(void) { return g_err; }
extern "C" int ep24_abi_version(void) { return EP24_ABI_VERSION; }
// always 0: kept so that version-3 callers keep binding (it told the product library from one that carried the removed kernel variants)
extern "C" int ep24_ab_variants(void) { return 0; }
