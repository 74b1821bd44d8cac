// Test-only probe of per-row frame origins (SE_CFG_STREAM_ROW_ORIGINS): every launcher that hands StreamCtx::origin or an origin
// argument to its kernels - launch_cln (the register, window and three-launch forms), launch_tcm_chain, and FullSubNet's
// launch_fsn_cum_fb / launch_fsn_cum_sb / launch_fsn_stream_apply - on device buffers the caller owns, under a chunk the caller opens with
// an origin pointer of its choice (null included).  A stream's state slots can be counted and read.  Every call is synchronised on both
// sides.  Plain C entry points for ctypes: tests/test_gpu_origin_kernels.py runs each form for three rows with origins and compares it,
// bit for bit, with the same launcher run row by row without.  Not linked into libse_engine.so.
#include "../blocks.h"
#include "../k_fullsubnet.h"
#include <memory>
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::unique_ptr<StreamScope> g_scope;      // the chunk published by orp_scope_open

struct Stream {
    StreamSlots slots;
    int B = 0;
};
struct Tcm {
    TcmBlock blk;
    ~Tcm() { blk.free(); }
};

template <typename F>
int guarded(F&& f) {
    try {
        SE_HIP(hipDeviceSynchronize());
        f();
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        g_scope.reset();
        set_stream_ctx(nullptr);
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* orp_last_error() { return g_err.c_str(); }

// ---- a frame-online stream of B rows: zero state, as a model's stream_begin leaves it
void* orp_stream_create(int B) {
    Stream* sm = nullptr;
    guarded([&] {
        sm = new Stream();
        sm->B = B;
        sm->slots.begin(B, 0);
    });
    return sm;
}
void orp_stream_destroy(void* h) {
    (void)hipDeviceSynchronize();
    g_scope.reset();
    delete static_cast<Stream*>(h);
}
int orp_slot_count(void* h) { return (int)static_cast<Stream*>(h)->slots.v.size(); }
long long orp_slot_bytes(void* h, int i) {
    const Stream* sm = static_cast<Stream*>(h);
    return i >= 0 && i < (int)sm->slots.v.size() ? (long long)sm->slots.v[i].second : -1;
}
int orp_slot_read(void* h, int i, void* host, long long bytes) {
    return guarded([&] {
        const Stream* sm = static_cast<Stream*>(h);
        SE_CHECK(i >= 0 && i < (int)sm->slots.v.size() && bytes == (long long)sm->slots.v[i].second, "orp_slot_read: no such slot / size");
        SE_HIP(hipMemcpy(host, sm->slots.v[i].first, (size_t)bytes, hipMemcpyDeviceToHost));
    });
}
// one chunk of the stream: H history columns + n new frames, first new GROUP frame t0, the rows' origins (device, [B] int32, or null);
// every launch below until orp_scope_close belongs to it (state slots are taken in call order)
int orp_scope_open(void* h, int H, int n, long long t0, const int32_t* origin_dev) {
    return guarded([&] {
        Stream* sm = static_cast<Stream*>(h);
        g_scope.reset();
        g_scope.reset(new StreamScope(sm->slots, H, n, (long)t0, sm->B, origin_dev));
    });
}
void orp_scope_close() { g_scope.reset(); }

// ---- launch_cln on a window x [B][C * F][T] of the open chunk (T = H + n); which of its forms runs follows from the sizes
int orp_cln(const float* x, float* y, const float* gain, const float* bias, const float* pre, const float* post, const float* fir, int K,
            int B, int C, int F, int T, const float* res) {
    return guarded([&] {
        SE_CHECK(stream_ctx(), "orp_cln: no chunk is open");
        launch_cln(x, y, gain, bias, pre, post, fir, K, B, C, F, T, 0, res);
    });
}

// ---- TCM blocks: a state dict in torch layout -> TcmBlock::load -> launch_tcm_chain on the open chunk
void* orp_sd_create() { return new StateDict(); }
void orp_sd_destroy(void* h) { delete static_cast<StateDict*>(h); }
void orp_sd_put(void* h, const char* key, const float* host, const long long* shape, int nd) {
    HostTensor t;
    for (int i = 0; i < nd; ++i) t.shape.push_back(shape[i]);
    t.data.assign(host, host + t.numel());
    (*static_cast<StateDict*>(h))[key] = std::move(t);
}
void* orp_tcm_create(void* sd, const char* prefix, int dil, const char* left, const char* right, int conv_idx, int fir_k, int ks, int gated) {
    Tcm* t = nullptr;
    guarded([&] {
        Tcm* p = new Tcm();
        try {
            const TrackedSD tsd(*static_cast<StateDict*>(sd));
            p->blk.load(tsd, prefix, dil, left, right, conv_idx, fir_k, ks, gated != 0);
        } catch (...) {
            delete p;
            throw;
        }
        t = p;
    });
    return t;
}
void orp_tcm_destroy(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<Tcm*>(h);
}
int orp_tcm_chain(void* const* blocks, int nblk, const float* x, float* y) {
    return guarded([&] {
        std::vector<const TcmStreamW*> f;
        std::vector<TcmFusedHeads> hd;
        std::vector<int> dil, K;
        for (int i = 0; i < nblk; ++i) {
            const TcmBlock& k = static_cast<const Tcm*>(blocks[i])->blk;
            SE_CHECK(k.sfused.w_in && k.nL.cum && k.nO.cum, "orp_tcm_chain: a block without the frame-online form");
            f.push_back(&k.sfused);
            hd.push_back(TcmFusedHeads{k.nL.s, k.nL.g, k.nL.b, k.firL, k.nR.s, k.nR.g, k.nR.b, k.firR, k.nO.s, k.nO.g, k.nO.b});
            dil.push_back(k.d);
            K.push_back(k.K);
        }
        launch_tcm_chain(f.data(), hd.data(), dil.data(), K.data(), nblk, x, y, 0);
    });
}

// ---- FullSubNet's frame-counting kernels (k_fullsubnet.h), with the origin argument the streaming model passes
int orp_fsn_cum_fb(const float* x, float* y, int n, int B, float* csum, int t_first, const int32_t* origin_dev) {
    return guarded([&] { launch_fsn_cum_fb(x, y, n, B, csum, t_first, 0, origin_dev); });
}
int orp_fsn_cum_sb(float* sb, int n, int S, float* csum, int t_first, const int32_t* origin_dev) {
    return guarded([&] { launch_fsn_cum_sb(sb, n, S, csum, t_first, 0, origin_dev); });
}
int orp_fsn_stream_apply(const float* maskT, const float* spec, float* est, int B, int Tw, int ns, int col0, int gt0, float p_out,
                         const int32_t* origin_dev) {
    return guarded([&] { launch_fsn_stream_apply(maskT, spec, est, B, Tw, ns, col0, gt0, p_out, 0, origin_dev); });
}

}  // extern "C"
