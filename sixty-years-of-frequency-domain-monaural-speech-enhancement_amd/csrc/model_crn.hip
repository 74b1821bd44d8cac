// CRN and LSTM (magnitude-mapping models with a 320/160 librosa front end) on the MI355X engine.
//
// Reference:
//   CRN/CRN.py:16-117 (crn_net: causal conv encoder x5 -> LSTM(1024,1024,2) -> deconv decoder x5, BN + ELU /
//     Softplus), decode loop CRN/crn_decode_vb.py:33-52.
//   LSTM/LSTM.py:14-28 (lstm_net: BatchNorm1d(161) -> LSTM(161,1024) -> LSTM(1024,1024,2) -> Linear + Softplus),
//     decode loop LSTM/lstm_decode_vb.py:33-52.
// Both map |X|^p_in -> enhanced magnitude and re-use the noisy phase (":49  est * exp(1j * phase)").
//
// Engine mapping: convs / deconvs are tap-table implicit GEMMs with BatchNorm folded and the activation in the
// epilogue, skip concatenations are two-source K loops; the 1024-wide LSTMs run time-major ([T][feature][B]) as one
// input-projection GEMM over all frames plus one fused GEMM + cell-update launch per frame.
#include "decode_frame.h"
#include "rnn.h"
#include <algorithm>
#include <vector>

namespace se {

namespace {

constexpr int NFFT = 320, HOP = 160, NBIN = 161;
constexpr int EC[5] = {16, 32, 64, 128, 256}, EF[5] = {80, 39, 19, 9, 4};          // CRN: encoder channels / bins per level
constexpr int DCo[5] = {128, 64, 32, 16, 1}, DF[5] = {9, 19, 39, 80, 161};         // ... decoder

// Feature-major LSTM layers ly[0..n) over x [I][T][B] (rnn.h run_fm), layer l into outs[l]: one clip - all layers as one
// wavefront launch (which writes the last layer's output only); up to 64 clips - the layers as a pipeline over chunks of frames,
// one cooperative launch per chunk; otherwise layer by layer
void lstm_layers_fm(const LstmBig* const* ly, int n, const float* x, float* G, float* cell, float* const* outs, int T, int B,
                    hipStream_t st, Profiler* pf) {
    if (B == 1 && lstm_stack_fm(ly, n, x, G, outs[n - 1], T, st, pf)) return;
    if (lstm_stack_chunked_fm(ly, n, x, G, cell, outs, T, B, st, pf)) return;
    for (int l = 0; l < n; ++l) {
        ly[l]->run_fm(x, G, cell, outs[l], T, B, st, pf);
        x = outs[l];
    }
}

// ------------------------------------------------------------------------------------------------ CRN
class Crn final : public Model {
  public:
    explicit Crn(EngineCtx& c) : Model(c) {}
    ~Crn() override {
        for (auto& p : enc) gc_free_plan(p);
        for (auto& p : dec) free_deconv_plan(p);
        for (auto& l : lstm) l.free();
    }
    StftGeom default_geom() const override { return StftGeom{NFFT, HOP, NFFT}; }

    void finalize(const TrackedSD& sd) override {
        for (int i = 0; i < 5; ++i) {   // CRN.py:35-71  pad(top 1 frame) + Conv2d((2,3),(1,2)) + BN + ELU
            const std::string p = "en.en_module." + std::to_string(i) + ".";
            DenseW w = conv_weights(sd.get(p + "1.weight", {EC[i], i ? EC[i - 1] : 1, 2, 3}), &sd.get(p + "1.bias", {EC[i]}), true);
            fold_bn(w, sd.get(p + "2.weight"), sd.get(p + "2.bias"), sd.get(p + "2.running_mean"), sd.get(p + "2.running_var"));
            enc[i] = make_conv_plan(w, 2, 0, 1, 1, 1, ACT_ELU, {}, EPI_ACT, 401);
        }
        for (int l = 0; l < 2; ++l) lstm[l].build(load_lstm(sd, "lstm.", l, "", 1024, 1024), ctx.max_batch);   // :20
        const int DC[5][2] = {{512, 128}, {256, 64}, {128, 32}, {64, 16}, {32, 1}};
        for (int i = 0; i < 5; ++i) {   // CRN.py:73-109  ConvTranspose2d((2,3),(1,2)) [+ left freq pad] + chomp + BN + ELU|Softplus
            const std::string p = "de.de_module." + std::to_string(i) + ".";
            DenseW w = deconv_weights(sd.get(p + "0.weight", {DC[i][0], DC[i][1], 2, 3}), &sd.get(p + "0.bias", {DC[i][1]}), true);
            const std::string bn = p + (i == 3 ? "3." : "2.");
            DenseW wz = w;                       // zero conv bias: the value BN sees on the zero-padded frequency row
            wz.bias.assign(wz.M, 0.f);
            fold_bn(w, sd.get(bn + "weight"), sd.get(bn + "bias"), sd.get(bn + "running_mean"), sd.get(bn + "running_var"));
            fold_bn(wz, sd.get(bn + "weight"), sd.get(bn + "bias"), sd.get(bn + "running_mean"), sd.get(bn + "running_var"));
            dec[i] = make_deconv_plan(w, 2, i == 3 ? -1 : 0, 0, i == 4 ? ACT_SOFTPLUS : ACT_ELU, {}, 401, DC[i][0] / 2,
                                      &wz.bias);
        }
    }

    void plan_buffers(int B, int T) override {
        cur.B = 0;
        bufs(B, T);
    }

    void forward(const float* in, const int64_t* shape, int ndim, float* out, hipStream_t st) override {
        SE_CHECK(ndim == 3 && shape[2] == NBIN, "CRN forward expects [B,T,161]");
        const int B = (int)shape[0], T = (int)shape[1];
        Bufs& b = bufs(B, T);
        // [B][T][F] -> [B][F][T]
        launch_transpose_akt(in, b.mag, T, B, NBIN, NBIN, (long)T * NBIN, T, (long)NBIN * T, st);
        network(b, st);
        launch_transpose_akt(b.D[5], out, NBIN, B, T, T, (long)NBIN * T, NBIN, (long)T * NBIN, st);
    }

    // causal end to end: eval BatchNorm is folded (decode_frame.h WorkFrames; the LSTMs walk the clip's own frames, Bufs::Tl)
    int frame_multiple() const override { return causal_frame_multiple(true); }
    void enhance(const float* wav, long pitch, int B, int L, float* out, long out_pitch, hipStream_t st) override {
        WorkFrames wf(ctx, B, L, L, 1 + L / HOP, st, true);
        const int Tw = wf.Tw, Ts = wf.Ts;
        Bufs& b = bufs(B, Tw);
        wf.own_frames(b.Tl);
        launch_rms_scale(wav, B, L, pitch, b.c, st);                                               // crn_decode_vb.py:34-35
        wf.zero_rows(b.mag, NBIN, st);
        launch_stft(ctx.geom, wav, pitch, B, L, L, b.c, ctx.p_in, b.spec, b.mag, Ts, Tw, st);       // :36-39
        network(b, st);                                                                            // :43
        launch_mag_phase(b.D[5], b.spec, b.est, B, NBIN, Tw, ctx.p_out, st);                       // :46-49
        launch_istft(ctx.geom, b.est, B, Ts, Tw, b.frames, b.c, out, out_pitch, L, st);             // :50-52
    }

    // ---- frame-online mode (model.h): every conv / deconv looks back exactly one frame (CRN.py:38 ConstantPad2d top 1 +
    // kernel 2 in time; :112-117 Chomp_T), the LSTMs carry (h, c)
    bool stream_supported() const override { return true; }
    StateLayout stream_layout() const override {
        StateLayout lay;
        for (long rows : stream_rows()) lay.hist.push_back({1, rows * STREAM_HC});      // [B][rows][HC]
        for (int l = 0; l < 2; ++l) lay.h[l] = lay.c[l] = {1024, 1};                    // [H][B]
        return lay;
    }
    void stream_begin(int B, int max_chunk, hipStream_t st) override {
        ss.begin(stream_layout(), B, st);
        (void)max_chunk;
    }
    void stream_bufs(int B, int n, float** spec, float** mag, float** est) override {
        Bufs& b = bufs(B, STREAM_HC + n);
        *spec = b.spec;
        *mag = b.mag;
        *est = b.est;
    }
    void stream_chunk(int B, int t0, int n, hipStream_t st, bool last) override {
        (void)last;
        SE_CHECK(ss.B == B && !ss.hist.empty(), "stream_chunk without stream_begin");
        const int HC = STREAM_HC, Tw = HC + n;
        Bufs& b = bufs(B, Tw);
        Profiler* pf = &ctx.prof;
        const std::vector<long> rows = stream_rows();
        float* tens[13] = {b.spec, b.mag, b.E[0], b.E[1], b.E[2], b.E[3], b.E[4], b.D[0], b.D[1], b.D[2], b.D[3], b.D[4], b.D[5]};
        // every layer only produces the new frames; the history columns its successor looks back on come from the state
        HistBatch hb;
        for (int k = 0; k < 13; ++k) hb.add(tens[k], ss.hist[k], rows[k]);
        launch_hist_batch(hb, B, Tw, HC, false, st);
        encoder(b, HC, st);
        launch_transpose_akt(b.E[4] + HC, b.X, B, 1024, n, 1024L * Tw, Tw, 1024L * B, B, st);
        lstm[0].run_stream(b.X, b.G, ss.c[0], ss.h[0], b.Hs[0], n, B, ss.first, st, pf);
        lstm[1].run_stream(b.Hs[0], b.G, ss.c[1], ss.h[1], b.Hs[1], n, B, ss.first, st, pf);
        launch_transpose_akt(b.Hs[1], b.D[0] + HC, n, 1024, B, 1024L * B, B, 1024L * Tw, Tw, st);
        decoder(b, HC, st);
        launch_mag_phase(b.D[5], b.spec, b.est, B, NBIN, Tw, ctx.p_out, st);     // history columns come out as last time
        launch_hist_batch(hb, B, Tw, HC, true, st);
        ss.first = false;
        (void)t0;
    }

  private:
    struct Bufs {
        int B = 0, T = 0;
        int Tl = 0;      // > 0: the clip's own frame count when the rows are zero-extended to T (offline equal-length batches)
        float *c, *spec, *mag, *est, *frames, *E[5], *D[6], *X, *G, *Hs[2], *cell;
    } cur;
    GCPlan enc[5];
    DeconvPlan dec[5];
    LstmBig lstm[2];
    StreamState ss;

  public:
    StreamState* stream_state() override { return &ss; }

  private:
    static std::vector<long> stream_rows() {      // rows (C * F) of spec, mag, E[0..4], D[0..5]
        return {2L * NBIN, NBIN, 16L * 80, 32L * 39, 64L * 19, 128L * 9, 256L * 4, 1024L, 128L * 9, 64L * 19, 32L * 39, 16L * 80,
                1L * 161};
    }

    Bufs& bufs(int B, int T) {
        if (cur.B == B && cur.T == T) return cur;
        Arena& a = ctx.arena;
        a.reset();
        Bufs b;
        b.B = B;
        b.T = T;
        const size_t BT = (size_t)B * T;
        b.c = a.alloc_f(B);
        b.spec = a.alloc_f(BT * 2 * NBIN);
        b.mag = a.alloc_f(BT * NBIN);
        b.est = a.alloc_f(BT * 2 * NBIN);
        b.frames = nullptr;      // the fused iSTFT keeps its frames in LDS (k_stft.hip); kept in the struct for the launcher signature
        for (int i = 0; i < 5; ++i) b.E[i] = a.alloc_f(BT * EC[i] * EF[i]);
        b.D[0] = a.alloc_f(BT * 1024);
        for (int i = 0; i < 5; ++i) b.D[i + 1] = a.alloc_f(BT * DCo[i] * DF[i]);
        b.X = a.alloc_f(BT * 1024);
        b.G = a.alloc_f(BT * 4096);
        b.Hs[0] = a.alloc_f(BT * 1024);
        b.Hs[1] = a.alloc_f(BT * 1024);
        b.cell = a.alloc_f((size_t)2 * 1024 * B);        // (one per layer: the chunked layer pipeline runs both at once)
        cur = b;
        return cur;
    }

    // b.mag [B][161][T] -> b.E[0..4], b.D[0] [B][256][4][T] + skips -> b.D[5] [B][1][161][T];  tb: first frame produced (0
    // offline, STREAM_HC in a frame-online chunk, whose history columns come from the state)
    void encoder(Bufs& b, int tb, hipStream_t st) {
        const int B = b.B, T = b.T;
        Act4 x = act4(b.mag, 1, NBIN, T);
        for (int i = 0; i < 5; ++i) {
            run_conv(enc[i], x, nullptr, b.E[i], EC[i], EF[i], B, T, T, st, &ctx.prof, nullptr, tb);
            x = act4(b.E[i], EC[i], EF[i], T);
        }
    }
    void decoder(Bufs& b, int tb, hipStream_t st) {
        const int B = b.B, T = b.T;
        int cin = 256, fin = 4;
        for (int i = 0; i < 5; ++i) {
            Act4 a0 = act4(b.D[i], cin, fin, T);
            Act4 a1 = act4(b.E[4 - i], cin, fin, T);
            run_deconv(dec[i], a0, &a1, b.D[i + 1], DCo[i], DF[i], B, T, T, st, &ctx.prof, nullptr, tb);
            cin = DCo[i];
            fin = DF[i];
        }
    }

    // b.mag [B][161][T] -> b.D[5] [B][1][161][T]
    void network(Bufs& b, hipStream_t st) {
        const int B = b.B, T = b.T;
        const int Tl = b.Tl > 0 ? b.Tl : T;      // frames the recurrent section walks (rows may be zero-extended: enhance())
        Profiler* pf = &ctx.prof;
        encoder(b, 0, st);
        // CRN.py:27-31  [B,256,T,4] -> [B,T,1024] -> LSTM x2 -> back;  engine: [B][1024][T] <-> [T][1024][B]
        if (lstm[0].fm_ok(B) && lstm[1].fm_ok(B)) {
            // feature-major [1024][T][B] (rnn.h run_fm): the two 4096 x 1024 input projections are full-width GEMMs
            launch_transpose_akt(b.E[4], b.X, B, 1024, Tl, 1024L * T, T, B, (long)Tl * B, st);
            const LstmBig* ly[2] = {&lstm[0], &lstm[1]};
            lstm_layers_fm(ly, 2, b.X, b.G, b.cell, b.Hs, Tl, B, st, pf);
            launch_transpose_akt(b.Hs[1], b.D[0], Tl, 1024, B, B, (long)Tl * B, 1024L * T, T, st);
        } else {
            launch_transpose_akt(b.E[4], b.X, B, 1024, Tl, 1024L * T, T, 1024L * B, B, st);
            lstm[0].run(b.X, b.G, b.cell, b.Hs[0], Tl, B, st, pf);
            lstm[1].run(b.Hs[0], b.G, b.cell, b.Hs[1], Tl, B, st, pf);
            launch_transpose_akt(b.Hs[1], b.D[0], Tl, 1024, B, 1024L * B, B, 1024L * T, T, st);
        }
        decoder(b, 0, st);
    }
};

// ------------------------------------------------------------------------------------------------ LSTM
class LstmNet final : public Model {
  public:
    explicit LstmNet(EngineCtx& c) : Model(c) {}
    ~LstmNet() override {
        for (auto& l : lstm) l.free();
        gc_free_plan(fc);
        gc_free_plan(fc_fm);
    }
    StftGeom default_geom() const override { return StftGeom{NFFT, HOP, NFFT}; }

    void finalize(const TrackedSD& sd) override {
        LstmW w0 = load_lstm(sd, "lstm1.", 0, "", NBIN, 1024);
        // LSTM.py:25  BatchNorm1d over the 161 features, folded into the first input projection
        fold_bn_input(w0.wih, sd.get("bn.weight", {NBIN}), sd.get("bn.bias", {NBIN}), sd.get("bn.running_mean", {NBIN}),
                      sd.get("bn.running_var", {NBIN}));
        lstm[0].build(w0, ctx.max_batch);
        lstm[1].build(load_lstm(sd, "lstm2.", 0, "", 1024, 1024), ctx.max_batch);
        lstm[2].build(load_lstm(sd, "lstm2.", 1, "", 1024, 1024), ctx.max_batch);
        DenseW f = linear_weights(sd.get("fc.0.weight", {NBIN, 1024}), &sd.get("fc.0.bias", {NBIN}));
        fc = make_pointwise_plan(f, ACT_SOFTPLUS, {}, ctx.max_batch);       // :20-22
        fc_fm = make_pointwise_plan(f, ACT_SOFTPLUS, {}, 4096);             // the same layer over feature-major rows
    }

    void plan_buffers(int B, int T) override {
        cur.B = 0;
        bufs(B, T);
    }

    void forward(const float* in, const int64_t* shape, int ndim, float* out, hipStream_t st) override {
        SE_CHECK(ndim == 3 && shape[2] == NBIN, "LSTM forward expects [B,T,161]");
        const int B = (int)shape[0], T = (int)shape[1];
        Bufs& b = bufs(B, T);
        if (fm(B)) {
            // [B][T][161] -> [161][T][B] and back
            launch_transpose_akt(in, b.X, B, T, NBIN, (long)T * NBIN, NBIN, (long)T * B, B, st);
            network_fm(b, st);
            launch_transpose_akt(b.Y, out, NBIN, T, B, (long)T * B, B, (long)T * NBIN, NBIN, st);
            return;
        }
        // [B][T*161] -> [T*161][B]
        launch_transpose_akt(in, b.X, B, 1, T * NBIN, (long)T * NBIN, 0, B, 0, st);
        network(b, st);
        launch_transpose_akt(b.Y, out, T * NBIN, 1, B, B, 0, (long)T * NBIN, 0, st);
    }

    void enhance(const float* wav, long pitch, int B, int L, float* out, long out_pitch, hipStream_t st) override {
        const int T = 1 + L / HOP;
        Bufs& b = bufs(B, T);
        launch_rms_scale(wav, B, L, pitch, b.c, st);                                               // lstm_decode_vb.py:35-36
        launch_stft(ctx.geom, wav, pitch, B, L, L, b.c, ctx.p_in, b.spec, b.mag, T, T, st);        // :37-38
        if (fm(B)) {
            launch_transpose_akt(b.mag, b.X, B, NBIN, T, (long)NBIN * T, T, B, (long)T * B, st);       // [B][161][T] -> [161][T][B]
            network_fm(b, st);                                                                         // :44
            launch_transpose_akt(b.Y, b.mag, T, NBIN, B, B, (long)T * B, (long)NBIN * T, T, st);
        } else {
            launch_transpose_akt(b.mag, b.X, B, NBIN, T, (long)NBIN * T, T, (long)NBIN * B, B, st);    // [B][161][T] -> [T][161][B]
            network(b, st);                                                                            // :44
            launch_transpose_akt(b.Y, b.mag, T, NBIN, B, (long)NBIN * B, B, (long)NBIN * T, T, st);
        }
        launch_mag_phase(b.mag, b.spec, b.est, B, NBIN, T, ctx.p_out, st);                         // :47-49
        launch_istft(ctx.geom, b.est, B, T, T, b.frames, b.c, out, out_pitch, L, st);              // :50-52
    }

    // ---- frame-online mode: the network is three unidirectional LSTMs + a per-frame Linear, so the state is (h, c) x 3
    bool stream_supported() const override { return true; }
    StateLayout stream_layout() const override {
        StateLayout lay;
        lay.hist.push_back({1, 2L * NBIN * STREAM_HC});      // spec [B][2][NBIN][HC]
        lay.hist.push_back({1, (long)NBIN * STREAM_HC});     // est magnitudes [B][NBIN][HC]
        for (int l = 0; l < 3; ++l) lay.h[l] = lay.c[l] = {1024, 1};      // [H][B]
        return lay;
    }
    void stream_begin(int B, int max_chunk, hipStream_t st) override {
        ss.begin(stream_layout(), B, st);
        (void)max_chunk;
    }
    void stream_bufs(int B, int n, float** spec, float** mag, float** est) override {
        Bufs& b = bufs(B, STREAM_HC + n);
        *spec = b.spec;
        *mag = b.mag;
        *est = b.est;
    }
    void stream_chunk(int B, int t0, int n, hipStream_t st, bool last) override {
        (void)last;
        SE_CHECK(ss.B == B && !ss.hist.empty(), "stream_chunk without stream_begin");
        const int HC = STREAM_HC, Tw = HC + n;
        Bufs& b = bufs(B, Tw);
        Profiler* pf = &ctx.prof;
        launch_hist_restore(b.spec, ss.hist[0], B, 2L * NBIN, Tw, HC, st);
        launch_transpose_akt(b.mag + HC, b.X, B, NBIN, n, (long)NBIN * Tw, Tw, (long)NBIN * B, B, st);      // new frames only
        lstm[0].run_stream(b.X, b.G, ss.c[0], ss.h[0], b.Hs[0], n, B, ss.first, st, pf);
        lstm[1].run_stream(b.Hs[0], b.G, ss.c[1], ss.h[1], b.Hs[1], n, B, ss.first, st, pf);
        lstm[2].run_stream(b.Hs[1], b.G, ss.c[2], ss.h[2], b.Hs[0], n, B, ss.first, st, pf);
        run_pointwise(fc, b.Hs[0], 1024L * B, B, b.Y, (long)NBIN * B, B, n, B, st, pf);
        launch_transpose_akt(b.Y, b.mag + HC, n, NBIN, B, (long)NBIN * B, B, (long)NBIN * Tw, Tw, st);
        launch_hist_restore(b.mag, ss.hist[1], B, NBIN, Tw, HC, st);          // estimated magnitudes of the last two frames
        launch_mag_phase(b.mag, b.spec, b.est, B, NBIN, Tw, ctx.p_out, st);
        launch_hist_save(b.spec, ss.hist[0], B, 2L * NBIN, Tw, HC, st);
        launch_hist_save(b.mag, ss.hist[1], B, NBIN, Tw, HC, st);
        ss.first = false;
        (void)t0;
    }

  private:
    struct Bufs {
        int B = 0, T = 0;
        float *c, *spec, *mag, *est, *frames, *X, *Y, *G, *Hs[2], *cell;
    } cur;
    LstmBig lstm[3];
    GCPlan fc, fc_fm;
    StreamState ss;

  public:
    StreamState* stream_state() override { return &ss; }

  private:

    Bufs& bufs(int B, int T) {
        if (cur.B == B && cur.T == T) return cur;
        Arena& a = ctx.arena;
        a.reset();
        Bufs b;
        b.B = B;
        b.T = T;
        const size_t BT = (size_t)B * T;
        b.c = a.alloc_f(B);
        b.spec = a.alloc_f(BT * 2 * NBIN);
        b.mag = a.alloc_f(BT * NBIN);
        b.est = a.alloc_f(BT * 2 * NBIN);
        b.frames = nullptr;      // the fused iSTFT keeps its frames in LDS (k_stft.hip); kept in the struct for the launcher signature
        b.X = a.alloc_f(BT * NBIN);
        b.Y = a.alloc_f(BT * NBIN);
        b.G = a.alloc_f(BT * 4096);
        b.Hs[0] = a.alloc_f(BT * 1024);
        b.Hs[1] = a.alloc_f(BT * 1024);
        b.cell = a.alloc_f((size_t)3 * 1024 * B);        // (one per layer: the chunked layer pipeline runs all three at once)
        cur = b;
        return cur;
    }

    bool fm(int B) const { return lstm[0].fm_ok(B) && lstm[1].fm_ok(B) && lstm[2].fm_ok(B); }
    // feature-major twin of network(): b.X [161][T][B] -> b.Y [161][T][B] (rnn.h run_fm)
    void network_fm(Bufs& b, hipStream_t st) {
        const int B = b.B, T = b.T;
        const long N = (long)T * B;
        Profiler* pf = &ctx.prof;
        const LstmBig* ly[3] = {&lstm[0], &lstm[1], &lstm[2]};
        float* outs[3] = {b.Hs[0], b.Hs[1], b.Hs[0]};
        lstm_layers_fm(ly, 3, b.X, b.G, b.cell, outs, T, B, st, pf);
        run_pointwise(fc_fm, b.Hs[0], 0, N, b.Y, 0, N, 1, (int)N, st, pf);
    }
    // b.X [T][161][B] -> b.Y [T][161][B]
    void network(Bufs& b, hipStream_t st) {
        const int B = b.B, T = b.T;
        Profiler* pf = &ctx.prof;
        lstm[0].run(b.X, b.G, b.cell, b.Hs[0], T, B, st, pf);
        lstm[1].run(b.Hs[0], b.G, b.cell, b.Hs[1], T, B, st, pf);
        lstm[2].run(b.Hs[1], b.G, b.cell, b.Hs[0], T, B, st, pf);
        run_pointwise(fc, b.Hs[0], 1024L * B, B, b.Y, (long)NBIN * B, B, T, B, st, pf);
    }
};

}  // namespace

std::unique_ptr<Model> make_crn(EngineCtx& ctx) { return std::unique_ptr<Model>(new Crn(ctx)); }
std::unique_ptr<Model> make_lstm(EngineCtx& ctx) { return std::unique_ptr<Model>(new LstmNet(ctx)); }

}  // namespace se
