// The wav2vec 2.0 handle (wav2vec2.hip) as the ASTRAL tokenizer (astral.hip) shares it: the tokenizer's SSL front IS this encoder,
// created with the stack's final LayerNorm switched off, and its window groups run through the same group methods.
#pragma once
#include "content_encoder.h"

namespace svc {

constexpr int WV_MAX_B = 64, WV_DEFAULT_GROUP = 16, WV_MAX_CONV = 8;

struct LenTab { int v[WV_MAX_CONV + 1][MAX_WIN]; };                // samples, then rows after each conv, per window

// rows after the first `upto` extractor convs of n samples in one piece
long wv_frames(const svc_w2v_config_t& c, long n, int upto = WV_MAX_CONV);
// the checks svc_w2v_frames / _rows / _n_windows make of a configuration (error set, prefixed with `who`)
int wv_check_cfg(const svc_w2v_config_t* c, const char* who);
// svc_w2v_create; final_ln false: encoder.layer_norm.* is neither required nor applied, the output is the residual stream
// ext null: the strict checks of svc_w2v_create; else svc_w2v_create_ex's (the base family: group-norm extractor, post-LN encoder)
int w2v_create(const svc_w2v_config_t* cfg, const svc_w2v_ext_t* ext, const svc_tensor_desc_t* weights, int n_weights, void* stream, bool final_ln,
               svc_w2v_t** out);

}  // namespace svc

struct svc_w2v {
    svc_w2v_config_t cfg;
    int dt = 0;                      // tap-GEMM dtype of the convs and linears: 0 fp16 (precision 1), 1 fp32 (precision 0)
    int group = svc::WV_DEFAULT_GROUP;
    svc::Arena wts, ws_fe, ws_enc;
    float* w0 = nullptr; float* b0 = nullptr;                           // conv0 [k0][C], bias
    svc::Lin conv[svc::WV_MAX_CONV], proj;
    float *cg[svc::WV_MAX_CONV] = {}, *cb[svc::WV_MAX_CONV] = {}, *pg = nullptr, *pb = nullptr;
    svc::half_t* pos16 = nullptr; float* pos32 = nullptr; float* posb = nullptr;
    svc::EncoderStack stack;
    // extractor workspace for cap_g windows of cap_n samples; encoder workspace for ecap_g windows of ecap_p rows
    int cap_g = 0; long cap_n = 0; int ecap_g = 0, ecap_p = 0;
    int Ls[svc::WV_MAX_CONV + 1] = {};    // row strides of the stage buffers of the current call (its longest window)
    long nstride = 0;
    float* wn = nullptr; double* part = nullptr; int* dlens = nullptr;
    void *actA = nullptr, *actB = nullptr; float* raw = nullptr;
    float *h32 = nullptr, *enc = nullptr, *acc32 = nullptr;
    svc::half_t* h16 = nullptr;
    // base family: group-norm extractor, samples as they are, positional-conv groups narrower than 64 channels
    bool group_norm = false, do_normalize = true;
    int pos_w = 64;                                                      // channels per positional-conv group (16, 32, 48, 64)
    double* gpart = nullptr;                                             // [MAX_WIN][WV_NBLK][k0 + k0 (k0 + 1) / 2] block partials
    float *gmean = nullptr, *gscale = nullptr, *gshift = nullptr;        // [MAX_WIN][16] tap means; [MAX_WIN][C] scale and shift of conv0
    float* hpad = nullptr;                                               // precision 0, pos_w < 64: h with every group zero-padded to 64 channels
    svc::StageTimer tm;
    int pack(const svc::StateDict& sd, const std::string& pre, hipStream_t st);
    int reserve_fe(int G, long nmax, hipStream_t st);
    int reserve_enc(int G, int P, hipStream_t st);
    int put_lens(const svc::LenTab& lt, hipStream_t st);
    int normalize_group(const float* wave, long Lrow, const svc::WinTab& wt, int G, float* dst, long stride, hipStream_t st);
    int features_group(const float* wnorm, long stride, int G, hipStream_t st);            // -> h32 (+ h16) [G][Ls[n_conv]][D]
    int posconv_group(const float* h, const svc::half_t* h16v, int G, int P, float* out, hipStream_t st);
    int encode_group(const float* h, const svc::half_t* h16v, int G, int P, float* out, hipStream_t st);
};
