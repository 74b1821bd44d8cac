// Test-only probe of the engine-lifetime scratch pool (common.h: device_scratch): libse_engine.so's objects linked once more, next to
// a record of every hand-out (scratch_set_log) that ctypes can read.  A test loads THIS library as the engine (SE_ENGINE_LIB) in a
// process of its own, decodes through the ordinary C ABI and reads which buffer went to which key, on which stream, and whether
// that stream was capturing (tests/test_gpu_two_engines.py).  The record is per thread and off outside scp_begin / scp_end; the
// engine's C ABI knows nothing of it.
#include "../common.h"
#include <vector>

using namespace se;

namespace {
thread_local std::vector<ScratchRec> g_log;
}

extern "C" {

void scp_begin() {
    g_log.clear();
    scratch_set_log(&g_log);
}
void scp_end() { scratch_set_log(nullptr); }
int scp_count() { return (int)g_log.size(); }
// record i -> out[5] = purpose, key, stream, buffer, capturing (addresses as integers); returns 0, or 1 when i is out of range
int scp_get(int i, long long* out) {
    if (i < 0 || i >= (int)g_log.size() || !out) return 1;
    const ScratchRec& r = g_log[(size_t)i];
    out[0] = r.purpose;
    out[1] = (long long)reinterpret_cast<intptr_t>(r.key);
    out[2] = (long long)reinterpret_cast<intptr_t>(r.stream);
    out[3] = (long long)reinterpret_cast<intptr_t>(r.p);
    out[4] = r.capturing;
    return 0;
}

}  // extern "C"
