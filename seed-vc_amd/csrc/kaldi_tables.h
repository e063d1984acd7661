// Host-side constants of the Kaldi fbank front-ends (CAMPPlus: campplus.hip, FSMN-VAD: vad.hip) in the tap-GEMM's weight
// layout: 25 ms frames at 16 kHz, 512-point DFT, Kaldi-mel triangles from 20 Hz to Nyquist.  The two front-ends differ in
// their window only, which stays with each of them.
#pragma once
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace svc {

constexpr int KALDI_NFFT = 512, KALDI_NB = KALDI_NFFT / 2 + 1;

// DFT basis [round_up(2 nb, 128)][nfft]: rows [0, nb) cos, rows [nb, 2 nb) -sin
inline std::vector<float> kaldi_dft_basis() {
    const int nfft = KALDI_NFFT, nb = KALDI_NB;
    std::vector<float> basis((size_t)round_up(2 * nb, 128) * nfft, 0.f);
    for (int k = 0; k < nb; ++k)
        for (int n = 0; n < nfft; ++n) {
            const double ang = 2.0 * M_PI * (double)(((long)k * n) % nfft) / (double)nfft;
            basis[(size_t)k * nfft + n] = (float)cos(ang);
            basis[(size_t)(nb + k) * nfft + n] = (float)(-sin(ang));
        }
    return basis;
}

// mel bank [round_up(bins, 128)][round_up(nb, 32)], fp32 arithmetic as torchaudio.compliance.kaldi.get_mel_banks
inline std::vector<float> kaldi_mel_bank(int bins) {
    const int nfft = KALDI_NFFT, nb = KALDI_NB;
    std::vector<float> mel((size_t)round_up(bins, 128) * round_up(nb, 32), 0.f);
    auto melf = [](float f) { return 1127.0f * logf(1.0f + f / 700.0f); };
    const float mlo = melf(20.0f), mhi = melf(8000.0f), delta = (mhi - mlo) / (float)(bins + 1);
    const long ldm = round_up(nb, 32);
    for (int b = 0; b < bins; ++b) {
        const float left = mlo + b * delta, center = mlo + (b + 1.0f) * delta, right = mlo + (b + 2.0f) * delta;
        for (int k = 0; k < nfft / 2; ++k) {
            const float m = melf(16000.0f / nfft * (float)k);
            const float up = (m - left) / (center - left), down = (right - m) / (right - center);
            mel[(size_t)b * ldm + k] = std::max(0.0f, std::min(up, down));
        }
    }
    return mel;
}

}  // namespace svc
