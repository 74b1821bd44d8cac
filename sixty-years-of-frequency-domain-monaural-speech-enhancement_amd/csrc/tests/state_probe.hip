// Test-only probe of the multi-segment copy kernel behind se_stream_save / se_stream_restore (k_stream_state.hip): one launch over
// a table the caller describes, on device buffers the caller owns, built into a device table as the engine builds it.  Plain C
// entry points for ctypes: tests/test_gpu_stream_state.py compares with numpy.  Not linked into libse_engine.so.
#include "../kernels.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
}

extern "C" {

const char* sp_last_error() { return g_err.c_str(); }
int sp_tile() { return STATE_TILE; }

// nfix flat segments (src[i] -> dst[i], len[i] floats) and, when win != 0, a window segment behind them: src[nfix] / dst[nfix] are
// its bases, win_rows its runs of win_len floats from column win_src_off (pitch win_src_pitch) to column win_dst_off (pitch
// win_dst_pitch).  *tiles (may be null) = the grid of the launch.
int sp_copy(const void* const* src, void* const* dst, const int* len, int nfix, int win, int win_rows, int win_len, long win_src_off,
            long win_dst_off, long win_src_pitch, long win_dst_pitch, long* tiles) {
    StateSeg* tab = nullptr;
    try {
        std::vector<StateSeg> v((size_t)nfix + (win ? 1 : 0));
        long t = 0;
        for (int i = 0; i < nfix; ++i) {
            StateSeg sg{};
            sg.src = static_cast<const float*>(src[i]);
            sg.dst = static_cast<float*>(dst[i]);
            sg.rows = 1;
            sg.len = len[i];
            sg.tile0 = (int)t;
            t += state_seg_tiles(1, len[i]);
            v[(size_t)i] = sg;
        }
        StateWindow w;
        if (win) {
            StateSeg sg{};
            sg.src = static_cast<const float*>(src[nfix]);
            sg.dst = static_cast<float*>(dst[nfix]);
            sg.rows = win_rows;
            sg.tile0 = (int)t;
            v[(size_t)nfix] = sg;
            w.src_off = win_src_off;
            w.dst_off = win_dst_off;
            w.src_pitch = win_src_pitch;
            w.dst_pitch = win_dst_pitch;
            w.rows = win_rows;
            w.len = win_len;
        }
        if (tiles) *tiles = t + (win ? state_seg_tiles(win_rows, win_len) : 0);
        SE_HIP(hipDeviceSynchronize());
        if (!v.empty()) {
            SE_HIP(hipMalloc(reinterpret_cast<void**>(&tab), v.size() * sizeof(StateSeg)));
            SE_HIP(hipMemcpy(tab, v.data(), v.size() * sizeof(StateSeg), hipMemcpyHostToDevice));
        }
        launch_stream_state_copy(tab, nfix, t, win ? nfix : -1, w, 0);
        SE_HIP(hipDeviceSynchronize());
        if (tab) (void)hipFree(tab);
        return 0;
    } catch (const std::exception& e) {
        if (tab) (void)hipFree(tab);
        g_err = e.what();
        return -1;
    }
}

}  // extern "C"
