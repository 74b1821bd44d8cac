// FullSubNet on the MI355X engine.
//
// Reference: FullSubNet/fullsubnet_net_sa/model.py:68-118 (Model.forward), base_model.py:13-42 (unfold),
// :197-209 (offline_laplace_norm), :212-240 (cumulative_laplace_norm), :242-255 (offline_gaussian_norm), :258-294
// (cumulative_layer_norm), selected at :296-308; sequence_model.py:66-84; constructor and decode loop
// FullSubNet/fullsubnet_sa_decode_vb.py:11-24, :37-72 (complex mask applied in the script, :56-61).
//
// Batch semantics: the reference only ever decodes B = 1 and its forward runs the training-time `drop_band`
// (model.py:101-104) whenever batch_size > 1; the engine therefore computes B INDEPENDENT batch-1 results (per-
// utterance normalisation statistics, no band dropping), see SURVEY.md 0.8.
//
// Engine mapping (time-major, sequences contiguous; la = look_ahead, W = (2 sbn + 1) + (2 fbn + 1), the script's 2 and 32):
//   full-band LSTM  : [T+la][257][B]     (B sequences, hidden 512)
//   sub-band LSTM   : [T+la][W][257*B]   (sequence s = n*B + b: sub-band n of utterance b, hidden 384) - the one
//                     place a recurrent step is a large GEMM (M = 1536, K = 384, N = 257*B), run on f32 MFMA with the
//                     LSTM cell fused in the epilogue.
//
// Shape: look_ahead (0..6) and fb_num_neighbors (0..15) are fields of the engine's flags (SE_CFG_FSN_LOOK_AHEAD / _FB_NEIGHBORS,
// include/se_engine.h); sb_num_neighbors (0..15) is read in finalize() from the width of sb_model.sequence_model.weight_ih_l0
// (model.py:50).  The workspace is planned after finalize() (se_engine_finalize), so bufs() sizes the sub-band input for the width the
// weights brought and nothing is planned for the widest one.
#include "decode_frame.h"
#include "rnn.h"
#include "k_fullsubnet.h"
#include "../../include/se_engine.h"

namespace se {

using namespace fsn;      // NBIN, LA_MAX, NEIGHBORS_MAX, sb_width, FSN_SUM_BLOCKS, FSN_EPS (k_fullsubnet.h)

namespace {

constexpr int NFFT = 512, HOP = 256;

class FullSubNet final : public Model {
  public:
    explicit FullSubNet(EngineCtx& c) : Model(c) {
        // (se_engine_create has checked both fields; 0 in the look-ahead field = the script's 2, as SE_CFG_REPEATS reads)
        const int laf = (int)((c.flags >> 22) & 7);
        la = laf ? laf - 1 : fsn::LA;
        fbn = (int)((c.flags >> 25) & 15);
    }
    ~FullSubNet() override {
        for (auto& l : fb) l.free();
        for (auto& l : sbl) l.free();
        gc_free_plan(fb_fc);
        gc_free_plan(sb_fc);
    }
    StftGeom default_geom() const override { return StftGeom{NFFT, HOP, NFFT}; }

    void finalize(const TrackedSD& sd) override {
        const int S = NBIN * ctx.max_batch;
        // sequence_model = "LSTM" (the decode script's choice, fullsubnet_sa_decode_vb.py:16) or "GRU" (sequence_model.py:36-43)
        const bool gru = (ctx.flags & SE_CFG_FSN_GRU) != 0;
        // norm_type (base_model.py:296-308; se_engine_create lets at most one of the three bits through)
        norm = (ctx.flags & SE_CFG_FSN_CUMULATIVE) ? NORM_CUM_LAPLACE
               : (ctx.flags & SE_CFG_FSN_GAUSSIAN) ? NORM_GAUSSIAN
               : (ctx.flags & SE_CFG_FSN_CUM_LAYERNORM) ? NORM_CUM_LAYERNORM : NORM_LAPLACE;
        is_gru = gru;
        // sb_num_neighbors from the sub-band model's input width I = (2 sbn + 1) + (2 fbn + 1) (model.py:50)
        {
            const std::string key = "sb_model.sequence_model.weight_ih_l0";
            SE_CHECK(sd.has(key), "FullSubNet: the state dict has no " + key);
            const HostTensor& wih = sd.get(key);
            const int I = wih.shape.size() == 2 ? (int)wih.shape[1] : -1;
            const int twice = I - 2 * fbn - 2;
            SE_CHECK(twice >= 0 && twice % 2 == 0 && twice <= 2 * NEIGHBORS_MAX,
                     "FullSubNet: " + key + " has an input width of " + std::to_string(I) + " with fb_num_neighbors = " + std::to_string(fbn) +
                         " (SE_CFG_FSN_FB_NEIGHBORS): the width is (2 sb_num_neighbors + 1) + (2 fb_num_neighbors + 1) with sb_num_neighbors "
                         "in 0..15");
            sbn = twice / 2;
            sbw = sb_width(sbn, fbn);
        }
        auto load = [&](const std::string& p, int layer, int I, int H) {
            return gru ? load_gru(sd, p, layer, "", I, H) : load_lstm(sd, p, layer, "", I, H);
        };
        fb[0].build(load("fb_model.sequence_model.", 0, NBIN, 512), ctx.max_batch, gru);
        fb[1].build(load("fb_model.sequence_model.", 1, 512, 512), ctx.max_batch, gru);
        fb_fc = make_pointwise_plan(linear_weights(sd.get("fb_model.fc_output_layer.weight", {NBIN, 512}),
                                                   &sd.get("fb_model.fc_output_layer.bias", {NBIN})),
                                    ACT_RELU, {}, ctx.max_batch);
        sbl[0].build(load("sb_model.sequence_model.", 0, sbw, 384), S, gru, true);
        sbl[1].build(load("sb_model.sequence_model.", 1, 384, 384), S, gru, true);
        sb_fc = make_pointwise_plan(linear_weights(sd.get("sb_model.fc_output_layer.weight", {2, 384}),
                                                   &sd.get("sb_model.fc_output_layer.bias", {2})),
                                    ACT_NONE, {}, S);
    }

    void plan_buffers(int B, int T) override {
        cur.B = 0;
        bufs(B, T);
    }

    void forward(const float* in, const int64_t* shape, int ndim, float* out, hipStream_t st) override {
        SE_CHECK(ndim == 4 && shape[1] == 1 && shape[2] == NBIN, "FullSubNet forward expects [B,1,257,T]");
        const int B = (int)shape[0], T = (int)shape[3];
        Bufs& b = bufs(B, T);
        network(b, in, st);
        launch_fsn_mask(b.maskBT, nullptr, out, B, T, 1.f, st, la);
    }

    void enhance(const float* wav, long pitch, int B, int L, float* out, long out_pitch, hipStream_t st) override {
        const int T = 1 + L / HOP;
        Bufs& b = bufs(B, T);
        launch_rms_scale(wav, B, L, pitch, b.c, st);                                               // :38-39
        launch_stft(ctx.geom, wav, pitch, B, L, L, b.c, ctx.p_in, b.spec, b.mag, T, T, st);        // :46-54
        network(b, b.mag, st);                                                                     // :56
        launch_fsn_mask(b.maskBT, b.spec, b.est, B, T, ctx.p_out, st, la);                                   // :57-66
        launch_istft(ctx.geom, b.est, B, T, T, b.frames, b.c, out, out_pitch, L, st);              // :69-72
    }

    // ---- frame-online mode (model.h), with one of the two cumulative norms only: every operator is then causal and the
    // network looks la = look_ahead frames ahead (model.py:79, :117 - the mask of frame t is the output of step t + la).  A chunk
    // of n new frames runs n network steps and finalises the estimate of frames [t0 - la, t0 + n - la) (stream_lag); the chunk
    // that ends the stream runs la more steps on the zero frames the offline forward pads (none with look_ahead = 0: every frame is
    // final at once, nothing is padded and nothing skipped).  From 16 clips on the first sub-band layer projects its W inputs inside the
    // step GEMM (K = 384 + W, rnn.h step_x): tests/test_gpu_fullsubnet_shapes.py decodes 16 clips at W = 2, 20 and 62.  State: the running sums of the
    // norms (per utterance / per sub-band sequence; the cumulative LayerNorm carries two of each, of x and of x^2), (h, c) of
    // the four LSTM layers, the last columns of spectrum and estimate.
    static constexpr int STREAM_TP_MAX = 64;      // longest window (frames incl. look-ahead) whose sub-band gate tensor is always kept
    bool stream_supported() const override { return causal() && !is_gru; }
    int stream_lag() const override { return la; }
    // history columns: the iSTFT looks back one frame and the estimate is final la frames late (engine_impl.h asks for la + 1); a
    // multiple of 4 as every model's - 4 up to look_ahead = 3 (the script's 2 included), 8 above
    int stream_hc() const override { return la <= 3 ? STREAM_HC : 2 * STREAM_HC; }
    void stream_begin(int B, int max_chunk, hipStream_t st) override {
        SE_CHECK(stream_hc() + max_chunk + la <= STREAM_TP_MAX,
                 "FullSubNet frame-online mode: chunks of at most " + std::to_string(STREAM_TP_MAX - stream_hc() - la) + " frames");
        ss.begin(stream_layout(), B, st);
    }
    StateLayout stream_layout() const override {
        StateLayout lay;
        lay.hist.push_back({1, 2L * NBIN * stream_hc()});      // spectrum [B][2][NBIN][HC]
        lay.hist.push_back({1, 2L * NBIN * stream_hc()});      // estimate
        // running sums of the full-band norm [B], then of the sub-band norm [S], sequence s = n * B + b; the cumulative LayerNorm
        // carries the sum of x and the sum of x^2 (slots of the same two shapes: the row operations know both)
        for (int k = 0; k < nsums(); ++k) lay.hist.push_back({1, 1});
        for (int k = 0; k < nsums(); ++k) lay.hist.push_back({NBIN, 1});
        for (int l = 0; l < 2; ++l) {
            lay.h[l] = lay.c[l] = {512, 1};                        // [H][B]
            lay.h[2 + l] = lay.c[2 + l] = {384L * NBIN, 1};        // [H][S]
        }
        return lay;
    }
    void stream_bufs(int B, int n, float** spec, float** mag, float** est) override {
        Bufs& b = bufs(B, stream_hc() + n);
        *spec = b.spec;
        *mag = b.mag;
        *est = b.est;
    }
    void stream_chunk(int B, int t0, int n, hipStream_t st, bool last) override {
        SE_CHECK(ss.B == B && ss.hist.size() == (size_t)(2 + 2 * nsums()), "stream_chunk without stream_begin");
        const int HC = stream_hc(), Tw = HC + n, S = NBIN * B;
        const int ns = n + (last ? la : 0);                 // network steps of this chunk
        SE_CHECK(Tw + la <= STREAM_TP_MAX, "FullSubNet frame-online mode: chunk too long");
        Bufs& b = bufs(B, Tw);
        Profiler* pf = &ctx.prof;
        launch_hist_restore(b.spec, ss.hist[0], B, 2L * NBIN, Tw, HC, st);
        launch_hist_restore(b.est, ss.hist[1], B, 2L * NBIN, Tw, HC, st);
        // magnitudes of the new frames, time-major [ns][257][B]; at the end of the stream la zero frames (model.py:79)
        launch_transpose_akt(b.mag + HC, b.magT, B, NBIN, n, (long)NBIN * Tw, Tw, (long)NBIN * B, B, st);
        if (last && la > 0) launch_fill(b.magT + (size_t)n * S, (long)la * S, 0.f, st);
        // (the engine hands a chunk at least one new frame, so ns >= 1 at every look-ahead)
        if (norm == NORM_CUM_LAYERNORM) launch_fsn_cln_fb(b.magT, b.xfb, ns, B, ss.hist[2], ss.hist[3], t0, st, ctx.stream_origin);
        else launch_fsn_cum_fb(b.magT, b.xfb, ns, B, ss.hist[2], t0, st, ctx.stream_origin);
        fb[0].run_stream(b.xfb, b.G, ss.c[0], ss.h[0], b.h[0], ns, B, ss.first, st, pf);
        fb[1].run_stream(b.h[0], b.G, ss.c[1], ss.h[1], b.h[1], ns, B, ss.first, st, pf);
        run_pointwise(fb_fc, b.h[1], 512L * B, B, b.fbo, (long)NBIN * B, B, ns, B, st, pf);
        launch_fsn_build_sb(b.magT, b.fbo, b.sb, B, ns, st, sbn, fbn);
        if (norm == NORM_CUM_LAYERNORM) launch_fsn_cln_sb(b.sb, ns, S, ss.hist[4], ss.hist[5], t0, st, ctx.stream_origin, sbw);
        else launch_fsn_cum_sb(b.sb, ns, S, ss.hist[3], t0, st, ctx.stream_origin, sbw);
        sbl[0].run_stream(b.sb, b.G, ss.c[2], ss.h[2], b.h[0], ns, S, ss.first, st, pf);
        sbl[1].run_stream(b.h[0], b.G, ss.c[3], ss.h[3], b.h[1], ns, S, ss.first, st, pf);
        run_pointwise(sb_fc, b.h[1], 384L * S, S, b.maskT, 2L * S, S, ns, S, st, pf);
        launch_fsn_stream_apply(b.maskT, b.spec, b.est, B, Tw, ns, HC - la, t0, ctx.p_out, st, ctx.stream_origin, la);
        launch_hist_save(b.spec, ss.hist[0], B, 2L * NBIN, Tw, HC, st);
        launch_hist_save(b.est, ss.hist[1], B, 2L * NBIN, Tw, HC, st);
        ss.first = false;
    }

  private:
    StreamState ss;

  public:
    StreamState* stream_state() override { return &ss; }

  private:
    enum NormKind { NORM_LAPLACE, NORM_CUM_LAPLACE, NORM_GAUSSIAN, NORM_CUM_LAYERNORM };
    NormKind norm = NORM_LAPLACE;
    bool is_gru = false;
    int la = fsn::LA, sbn = fsn::SBN, fbn = 0, sbw = fsn::SBW;      // look_ahead, the neighbour counts, the sub-band input's width
    bool causal() const { return norm == NORM_CUM_LAPLACE || norm == NORM_CUM_LAYERNORM; }
    int nsums() const { return norm == NORM_CUM_LAYERNORM ? 2 : 1; }      // running sums a stream carries per norm
    struct Bufs {
        int B = 0, T = 0;
        float *c, *spec, *mag, *est, *frames, *mu, *mu2, *part;
        float *stat = nullptr, *stat2 = nullptr;      // offline_gaussian_norm: (mean, std + 1e-5) [2][B] of the full band, of the sub bands
        double* dpart = nullptr;                      // ... and the float64 partials of its two moments [FSN_SUM_BLOCKS][2][B]
        float *magT, *xfb, *G, *h[2], *cell, *fbo, *sb, *maskT, *maskBT, *hz;
    } cur;
    LstmBig fb[2], sbl[2];
    GCPlan fb_fc, sb_fc;

    Bufs& bufs(int B, int T) {
        if (cur.B == B && cur.T == T) return cur;
        Arena& a = ctx.arena;
        a.reset();
        Bufs b;
        b.B = B;
        b.T = T;
        const size_t BT = (size_t)B * T, Tp = T + la, S = (size_t)NBIN * B;
        b.c = a.alloc_f(B);
        b.mu = a.alloc_f(B);
        b.mu2 = a.alloc_f(B);
        b.part = a.alloc_f((size_t)FSN_SUM_BLOCKS * B);
        b.spec = a.alloc_f(BT * 2 * NBIN);
        b.mag = a.alloc_f(BT * NBIN);
        b.est = a.alloc_f(BT * 2 * NBIN);
        b.frames = nullptr;      // the fused iSTFT keeps its frames in LDS (k_stft.hip); kept in the struct for the launcher signature
        b.magT = a.alloc_f(Tp * S);
        b.xfb = a.alloc_f(Tp * S);
        b.fbo = a.alloc_f(Tp * S);
        b.sb = a.alloc_f(Tp * sbw * S);
        // gate pre-activations: the full-band layers' [Tp][2048][B]; the sub-band layers' [Tp][1536][S] only when they do not
        // project their inputs inside the step GEMM (51 GB at 128 clips)
        // (a frame-online window - a few frames - always keeps them: the streamed steps go through LstmBig::run_stream)
        const bool sb_gates = !(fuse_x_on(B) && sbl[0].has_x && sbl[1].has_x) || (causal() && Tp <= STREAM_TP_MAX);
        b.G = a.alloc_f(sb_gates ? Tp * 1536 * S : Tp * 2048 * (size_t)B);
        b.h[0] = a.alloc_f(Tp * 384 * S);               // also the full-band hidden [Tp][512][B]
        b.h[1] = a.alloc_f(Tp * 384 * S);
        b.cell = a.alloc_f(384 * S + 512 * (size_t)B);
        b.hz = a.alloc_f(384 * S);                      // zeros: h_{-1} of the sub-band layer that projects its own input
        b.maskT = a.alloc_f(Tp * 2 * S);
        b.maskBT = a.alloc_f(Tp * 2 * S);
        if (norm == NORM_GAUSSIAN) {
            b.stat = a.alloc_f(2 * (size_t)B);
            b.stat2 = a.alloc_f(2 * (size_t)B);
            b.dpart = static_cast<double*>(a.alloc((size_t)FSN_SUM_BLOCKS * 2 * B * sizeof(double)));
        }
        cur = b;
        return cur;
    }

    bool graph_capturable() const override { return false; }     // sub-band halves run on two streams
    // the sub-band layers project their inputs inside the step GEMM (rnn.h step_x) from 16 clips on; below, a step launch is a
    // latency-bound K loop of a few workgroups and a K of 768 instead of 384 costs more than the batched projection into a
    // [T][4H][S] gate tensor it replaces (one clip: 38 vs 30 utt/s)
    static bool fuse_x_on(int B) { return B >= 16; }

    // mag [B][257][T] -> maskBT [n*B+b][2][T+la]
    void network(Bufs& b, const float* mag, hipStream_t st) {
        const int B = b.B, T = b.T, Tp = T + la, S = NBIN * B;
        Profiler* pf = &ctx.prof;
        // ---- full-band model (model.py:84-85): utterance-mean normalisation, LSTM(257->512)x2, Linear + ReLU
        const Ragged* rg = ragged_ctx();
        const int* tlen = rg ? rg->tlen : nullptr;
        if (norm == NORM_LAPLACE) launch_fsn_mean(mag, B, NBIN * T, (float)NBIN * Tp, b.mu, tlen, st, la);
        if (la > 0) launch_fill(b.magT + (size_t)T * S, (long)la * S, 0.f, st);                         // look-ahead pad :79 (a kernel, not a memset node: graph-replay safe)
        launch_transpose_akt(mag, b.magT, B, NBIN, T, (long)NBIN * T, T, (long)NBIN * B, B, st);
        const long nfb = (long)Tp * S;
        // (cumulative norm, ragged rows: frames >= tlen[b] are zeros - the STFT wrote them - and everything is causal, so a
        // row's own frames and its la look-ahead frames see exactly what the clip decoded alone sees)
        switch (norm) {
            case NORM_CUM_LAPLACE: launch_fsn_cum_fb(b.magT, b.xfb, Tp, B, nullptr, 0, st); break;
            case NORM_CUM_LAYERNORM: launch_fsn_cln_fb(b.magT, b.xfb, Tp, B, nullptr, nullptr, 0, st); break;
            case NORM_GAUSSIAN:
                // both moments of the padded magnitudes in one float64 pass (a ragged row: its own tlen[b] + la frames), then the apply
                launch_fsn_moments(b.magT, (long)Tp * NBIN, B, b.dpart, tlen, NBIN, st, la);
                launch_fsn_finish_gauss(b.dpart, b.stat, (long)Tp * NBIN, B, tlen, NBIN, st, la);
                launch_fsn_gauss_apply(b.magT, b.xfb, nfb, B, b.stat, st);
                break;
            case NORM_LAPLACE: launch_fsn_scale(b.magT, b.xfb, nfb, B, b.mu, st); break;
        }
        fb[0].run(b.xfb, b.G, b.cell, b.h[0], Tp, B, st, pf);
        fb[1].run(b.h[0], b.G, b.cell, b.h[1], Tp, B, st, pf);
        run_pointwise(fb_fc, b.h[1], 512L * B, B, b.fbo, (long)NBIN * B, B, Tp, B, st, pf);
        // ---- sub-band input (:88-97): unfold(noisy, sbn) ++ unfold(fb_out, fbn), normalised by its utterance mean
        launch_fsn_build_sb(b.magT, b.fbo, b.sb, B, Tp, st, sbn, fbn);
        const long frame_rows = (long)sbw * NBIN, rows = (long)Tp * frame_rows;
        SE_CHECK(B <= 256, "FullSubNet batch per call is limited to 256 utterances");
        if (norm == NORM_CUM_LAPLACE) {
            launch_fsn_cum_sb(b.sb, Tp, S, nullptr, 0, st, nullptr, sbw);
        } else if (norm == NORM_CUM_LAYERNORM) {
            launch_fsn_cln_sb(b.sb, Tp, S, nullptr, nullptr, 0, st, nullptr, sbw);
        } else if (norm == NORM_GAUSSIAN) {
            // the sub-band tensor is read once for its statistics, as the Laplace path reads it, and normalised in place
            launch_fsn_moments(b.sb, rows, B, b.dpart, tlen, frame_rows, st, la);
            launch_fsn_finish_gauss(b.dpart, b.stat2, rows, B, tlen, frame_rows, st, la);
            launch_fsn_gauss_apply(b.sb, b.sb, rows * B, B, b.stat2, st);
        } else {
            launch_fsn_colsum(b.sb, rows, B, b.part, tlen, st, frame_rows, la);
            launch_fsn_finish_mean(b.part, b.mu2, (float)rows, B, tlen, st, frame_rows, la);
            const long nsb = rows * B;
            launch_fsn_scale(b.sb, b.sb, nsb, B, b.mu2, st);
        }
        SE_HIP(hipGetLastError());
        // ---- sub-band model (:106-114): LSTM(W->384)x2 over 257*B sequences, Linear(384->2)
        // The 257 * B sequences are independent: two column halves run on two streams, so that the short per-step
        // launches of one half (2 block rounds, every block in the same phase) overlap the other half's instead of
        // leaving the matrix pipes idle during everybody's prologue / epilogue.
        float* cell = b.cell + 512 * (size_t)B;
        static const int parts_env = getenv("SE_FSN_SPLIT") ? atoi(getenv("SE_FSN_SPLIT")) : 2;
        const int parts = std::max(1, std::min({parts_env, 1 + EngineCtx::MAX_AUX, S / 256}));
        const int Sp = ((S + parts - 1) / parts + 127) / 128 * 128;           // columns per part (tile aligned)
        const bool fuse_x = fuse_x_on(B);
        const bool l0x = fuse_x && sbl[0].has_x;
        if (l0x) launch_fill(b.hz, 384L * S, 0.f, st);
        auto part = [&](int c0, int Sn, hipStream_t s, Profiler* p) {
            if (l0x) sbl[0].run_cols_x(b.sb, (long)sbw * S, cell, b.hz, b.h[0], 384L * S, 1, Tp, S, c0, Sn, s, p);
            else sbl[0].run_cols(b.sb, (long)sbw * S, b.G, cell, b.h[0], 384L * S, 1, Tp, S, c0, Sn, s, p);
            if (fuse_x && sbl[1].has_x) sbl[1].run_cols_x(b.h[0], 384L * S, cell, b.hz, b.h[1], 384L * S, 1, Tp, S, c0, Sn, s, p);
            else sbl[1].run_cols(b.h[0], 384L * S, b.G, cell, b.h[1], 384L * S, 1, Tp, S, c0, Sn, s, p);
            run_pointwise(sb_fc, b.h[1] + c0, 384L * S, S, b.maskT + c0, 2L * S, S, Tp, Sn, s, p);
        };
        Fork fk(ctx, st, true);      // (one part: no auxiliary stream is asked for, Sp >= S)
        for (int i = 1; i < parts && i * Sp < S; ++i) {
            part(i * Sp, std::min(Sp, S - i * Sp), fk.to(i - 1), fk.prof(i - 1));
            fk.done(i - 1);
        }
        part(0, std::min(Sp, S), st, pf);
        for (int i = 1; i < parts && i * Sp < S; ++i) fk.join(i - 1);
        // [Tp][2][S] -> [S][2][Tp]
        launch_transpose_akt(b.maskT, b.maskBT, Tp, 2, S, 2L * S, S, 2L * Tp, Tp, st);
    }
};

}  // namespace

std::unique_ptr<Model> make_fullsubnet(EngineCtx& ctx) { return std::unique_ptr<Model>(new FullSubNet(ctx)); }

}  // namespace se
