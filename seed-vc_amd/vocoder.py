"""Host-side mirrors of the reference vocoders over the C ABI.

`BigVGAN(h, state_dict)(mel) -> (B, 1, L)` mirrors `BigVGAN.forward` (modules/bigvgan/bigvgan.py:360-386; the
drivers call it as `vocoder_fn(vc_target.float())`, inference.py:506, and `.squeeze()` the result).
`HiFT(cfg, state_dict)(mel) -> (B, L)` mirrors `HiFTGenerator.forward` / `.inference`
(modules/hifigan/generator.py:400-436,452-454).  `precision`: "fp32" = exact fp32 MFMA, "fp16x3" = split hi/lo fp16
operands with three MFMA products per step (fp32-class accuracy, faster), "fp16p8" = the same split with the two
correction products of the long stride-1 convs in ONE block-scaled fp8 MFMA (waveform RMS ~1e-5: inside the 1e-4 bound
with margin, faster again), "fp16" = plain fp16 operands (2.4e-4: outside the bound, reported only).  HiFT's random draws (SineGen phases and noise,
generator.py:208-222) are drawn here with torch when the caller does not pass them; with `seeds=` (one 64-bit seed per
utterance) they are drawn on the device inside the source kernel instead and no (B, nh, S * up) tensor exists.

"fp16p8" has a fixed operand window (the fp8 correction bytes carry no activation scale and one weight scale per layer);
outside it a conv silently degrades to plain-fp16 operand error.  `calibrate(...)` measures, on the caller's own weights and
material, how much each candidate conv's correction bytes lose and vetoes the convs that lose more than `tau`: a vetoed conv
runs the fp16x3 form.  The vetoes are the handle's `precision_plan` ({state-dict prefix: bool}); it can be stored next to a
checkpoint and set again without calibration data.  The empty plan (the default) is plain "fp16p8", the full plan gives the
bits of "fp16x3"; no plan depends on the batch.
"""
import ctypes as C
import math

import torch

from . import _lib
from .specs import bigvgan_total_upsample, hift_total_upsample


PRECISIONS = {"fp32": 0, "fp16": 1, "fp16x3": 2, "fp16p8": 3}
DEFAULT_TAU = 2.0 ** -6     # calibrate's veto threshold on the loss ratios


class _PrecisionPlan:
    """The precision plan of an fp16p8 handle over svc_<voc>_plan_* (include/seedvc_hip.h)."""
    _voc = None     # "bigvgan" | "hift"

    def _plan(self, name):
        return getattr(_lib.lib(), f"svc_{self._voc}_{name}")

    def plan_names(self):
        """State-dict prefixes of the p8 candidate convs, in plan order (an "fp16p8" handle only)."""
        n = self._plan("plan_size")(self._h)
        if n < 0:
            raise RuntimeError('the precision plan belongs to a precision="fp16p8" handle')
        return [self._plan("plan_name")(self._h, i).decode() for i in range(n)]

    @property
    def precision_plan(self):
        """{prefix: vetoed} for every candidate conv; a vetoed conv runs the fp16x3 form instead of fp16 + fp8 corrections."""
        names = self.plan_names()
        veto = (C.c_uint8 * max(len(names), 1))()
        _lib.check(self._plan("plan_get")(self._h, veto, len(names)))
        return {k: bool(veto[i]) for i, k in enumerate(names)}

    @precision_plan.setter
    def precision_plan(self, plan):
        names = self.plan_names()
        unknown = sorted(set(plan) - set(names))
        if unknown:
            raise KeyError(f"precision_plan: not a p8 candidate of this model: {unknown}")
        cur = self.precision_plan
        cur.update({k: bool(v) for k, v in plan.items()})
        veto = (C.c_uint8 * max(len(names), 1))(*[int(cur[k]) for k in names])
        _lib.check(self._plan("plan_set")(self._h, veto, len(names)))

    def reset_plan(self):
        """Clears every veto: plain fp16p8 again."""
        _lib.check(self._plan("plan_reset")(self._h))

    def _report(self, names, rows):
        from .ops import census_dict
        out = []
        for k, r in zip(names, rows):
            d = {"index": r.index, "name": k, "veto": bool(r.veto), "L": r.L, "rho": r.rho, "eta": r.eta, "omega_hi": r.omega_hi,
                 "omega_lo": r.omega_lo}
            d.update(census_dict(r.census))
            out.append(d)
        return out

    @staticmethod
    def _lens_host(lens, B, who):
        if lens is None:
            return None
        lens = _lib.int_list(lens)
        if len(lens) != B:
            raise ValueError(f"{who}: lens has {len(lens)} entries, the batch has {B} utterances")
        return _lib.i32_host(lens)


class BigVGAN(_PrecisionPlan):
    _voc = "bigvgan"

    def __init__(self, h, state_dict, device="cuda:0", precision="fp16p8"):
        self.h = h
        self.device = torch.device(device)
        self.total_up = bigvgan_total_upsample(h)
        c = _lib.BigVGANConfig()
        c.num_mels = h["num_mels"]
        c.upsample_initial_channel = h["upsample_initial_channel"]
        c.num_upsamples = len(h["upsample_rates"])
        c.num_kernels = len(h["resblock_kernel_sizes"])
        for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
            c.upsample_rates[i], c.upsample_kernel_sizes[i] = u, k
        for j, (k, d) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            c.resblock_kernel_sizes[j] = k
            for e in range(3):
                c.resblock_dilation_sizes[j][e] = d[e]
        c.use_tanh_at_final = int(h.get("use_tanh_at_final", True))
        c.use_bias_at_final = int(h.get("use_bias_at_final", True))
        c.snake_logscale = int(h["snake_logscale"])
        c.snakebeta = int(h["activation"] == "snakebeta")
        c.precision = PRECISIONS[precision]
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            _lib.check(_lib.lib().svc_bigvgan_create(C.byref(c), descs, n, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    def set_microbatch(self, n):
        """Utterances per internal pass (0 = library default); the output does not depend on it."""
        _lib.check(_lib.lib().svc_bigvgan_set_microbatch(self._h, int(n)))

    @torch.inference_mode()
    def __call__(self, mel, lens=None):
        """mel (B, num_mels, S) -> (B, 1, S * up).  lens (list / LongTensor of B ints, 0 <= lens[b] <= S): a ragged batch in
        one call -- out[b, 0, :lens[b] * up] is the waveform of mel[b, :, :lens[b]] run alone, the rest of the row is zero,
        and frames at and above lens[b] may hold anything (svc_bigvgan_forward_ragged in include/seedvc_hip.h)."""
        B, _, S = mel.shape
        if lens is not None:
            lens = _lib.int_list(lens)
            if len(lens) != B:
                raise ValueError(f"BigVGAN: lens has {len(lens)} entries, the batch has {B} utterances")
        with torch.cuda.device(self.device):
            mel = _lib.f32c(mel, self.device)
            out = torch.empty(B, 1, S * self.total_up, device=self.device, dtype=torch.float32)
            if lens is None:
                _lib.check(_lib.lib().svc_bigvgan_forward(self._h, _lib.ptr(mel), B, S, _lib.ptr(out), _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().svc_bigvgan_forward_ragged(self._h, _lib.ptr(mel), _lib.i32_host(lens), B, S, _lib.ptr(out),
                                                                 _lib.stream_ptr()))
        return out

    forward = __call__

    @torch.inference_mode()
    def calibrate(self, mel, lens=None, tau=DEFAULT_TAU):
        """Calibrates the precision plan on mel (B, num_mels, S) [lens: B ints in [1, S]]: one fp16x3 forward with a range
        census of every candidate conv's operand planes, combined with the weight census; a conv whose loss ratios rho, eta
        or omega exceed tau is vetoed, and the vetoes are ORed into the plan (`svc_bigvgan_calibrate`).  Returns one report
        row (dict) per candidate: name, veto (this call's decision), rho, eta, omega_hi, omega_lo, L, the counts, max_hi."""
        B, _, S = mel.shape
        names = self.plan_names()
        rows = (_lib.PlanRow * max(len(names), 1))()
        lens_keep = self._lens_host(lens, B, "BigVGAN.calibrate")
        with torch.cuda.device(self.device):
            mel = _lib.f32c(mel, self.device)
            _lib.check(_lib.lib().svc_bigvgan_calibrate(self._h, _lib.ptr(mel), lens_keep, B, S, float(tau), rows, len(names),
                                                        _lib.stream_ptr()))
        return self._report(names, rows)

    def close(self):
        if self._h:
            _lib.lib().svc_bigvgan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HiFT(_PrecisionPlan):
    _voc = "hift"

    def __init__(self, cfg, state_dict, device="cuda:0", precision="fp16p8"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.total_up = hift_total_upsample(cfg)
        c = _lib.HiftConfig()
        c.in_channels, c.base_channels = cfg["in_channels"], cfg["base_channels"]
        c.nb_harmonics, c.sampling_rate = cfg["nb_harmonics"], cfg["sampling_rate"]
        c.nsf_alpha, c.nsf_sigma = cfg["nsf_alpha"], cfg["nsf_sigma"]
        c.nsf_voiced_threshold = cfg["nsf_voiced_threshold"]
        c.num_upsamples = len(cfg["upsample_rates"])
        for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            c.upsample_rates[i], c.upsample_kernel_sizes[i] = u, k
        c.istft_n_fft, c.istft_hop = cfg["istft_n_fft"], cfg["istft_hop"]
        c.num_kernels = len(cfg["resblock_kernel_sizes"])
        for j, (k, d) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            c.resblock_kernel_sizes[j] = k
            for e in range(3):
                c.resblock_dilation_sizes[j][e] = d[e]
        for j, (k, d) in enumerate(zip(cfg["source_resblock_kernel_sizes"], cfg["source_resblock_dilation_sizes"])):
            c.source_resblock_kernel_sizes[j] = k
            for e in range(3):
                c.source_resblock_dilation_sizes[j][e] = d[e]
        c.lrelu_slope, c.audio_limit = cfg["lrelu_slope"], cfg["audio_limit"]
        c.f0_cond_channels = cfg["f0_cond_channels"]
        c.precision = PRECISIONS[precision]
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            _lib.check(_lib.lib().svc_hift_create(C.byref(c), descs, n, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    def set_microbatch(self, n):
        """Utterances per internal pass (0 = library default); the output does not depend on it."""
        _lib.check(_lib.lib().svc_hift_set_microbatch(self._h, int(n)))

    @torch.inference_mode()
    def __call__(self, x, f0=None, phase0=None, noise=None, return_f0=False, lens=None, seeds=None):
        """x (B, 80, S) -> (B, S * up) [, f0 (B, S)].  lens (list / LongTensor of B ints, 0 <= lens[b] <= S): a ragged batch in
        one call -- out[b, :lens[b] * up] is the waveform of x[b, :, :lens[b]] run alone with f0[b, :lens[b]], phase0[b] and
        noise[b, :, :lens[b] * up] (the draws of the run alone), the rest of the row and of the returned f0 is zero, and
        frames, f0 values and noise samples past an utterance's end may hold anything (svc_hift_forward_ragged in
        include/seedvc_hip.h).  Draws made here have the same shapes with and without lens.
        seeds (B integers in [0, 2^64), exclusive with phase0 / noise): utterance b uses the draws of seeds[b], made inside
        the source kernel (`svc_hift_forward_seeded`; `noise_draws` returns them); with lens, row b is utterance b run alone
        with its seed, bit for bit."""
        B, _, S = x.shape
        if seeds is not None and (phase0 is not None or noise is not None):
            raise ValueError("HiFT: give seeds or phase0 / noise, not both")
        seeds_keep = _lib.seeds_host(seeds, B, "HiFT") if seeds is not None else None
        if lens is not None:
            lens = _lib.int_list(lens)
            if len(lens) != B:
                raise ValueError(f"HiFT: lens has {len(lens)} entries, the batch has {B} utterances")
        nh = self.cfg["nb_harmonics"] + 1
        Lw = S * self.total_up
        dev = self.device
        with torch.cuda.device(dev):
            mel = _lib.f32c(x, dev)
            if seeds is None:
                if phase0 is None:     # Uniform(-pi, pi).sample((B, nh, 1)): generator.py:208-209
                    phase0 = (torch.rand(B, nh, 1, device=dev) * 2 - 1) * math.pi
                if noise is None:      # torch.randn_like(sine_waves): generator.py:222
                    noise = torch.randn(B, nh, Lw, device=dev)
                phase0, noise = _lib.f32c(phase0, dev), _lib.f32c(noise, dev)
            f0t = _lib.f32c(f0, dev) if f0 is not None else None
            out = torch.empty(B, Lw, device=dev, dtype=torch.float32)
            f0_out = torch.empty(B, S, device=dev, dtype=torch.float32) if return_f0 else None
            lens_keep = _lib.i32_host(lens) if lens is not None else None
            args = (B, S, _lib.ptr(out), _lib.ptr(f0_out), _lib.stream_ptr())
            if seeds is not None:
                rc = _lib.lib().svc_hift_forward_seeded(self._h, _lib.ptr(mel), lens_keep, _lib.ptr(f0t), seeds_keep, *args)
            elif lens is None:
                rc = _lib.lib().svc_hift_forward(self._h, _lib.ptr(mel), _lib.ptr(f0t), _lib.ptr(phase0), _lib.ptr(noise), *args)
            else:
                rc = _lib.lib().svc_hift_forward_ragged(self._h, _lib.ptr(mel), lens_keep, _lib.ptr(f0t), _lib.ptr(phase0),
                                                        _lib.ptr(noise), *args)
            _lib.check(rc)
        return (out, f0_out) if return_f0 else out

    forward = __call__
    inference = __call__

    @torch.inference_mode()
    def calibrate(self, x, f0=None, phase0=None, noise=None, lens=None, tau=DEFAULT_TAU):
        """BigVGAN.calibrate for HiFT (`svc_hift_calibrate`): x (B, 80, S), f0 / phase0 / noise as in `__call__` (drawn here with
        torch when not given; f0 None = the model's predictor)."""
        B, _, S = x.shape
        nh, Lw, dev = self.cfg["nb_harmonics"] + 1, S * self.total_up, self.device
        names = self.plan_names()
        rows = (_lib.PlanRow * max(len(names), 1))()
        lens_keep = self._lens_host(lens, B, "HiFT.calibrate")
        with torch.cuda.device(dev):
            mel = _lib.f32c(x, dev)
            if phase0 is None:
                phase0 = (torch.rand(B, nh, 1, device=dev) * 2 - 1) * math.pi
            if noise is None:
                noise = torch.randn(B, nh, Lw, device=dev)
            phase0, noise = _lib.f32c(phase0, dev), _lib.f32c(noise, dev)
            f0t = _lib.f32c(f0, dev) if f0 is not None else None
            _lib.check(_lib.lib().svc_hift_calibrate(self._h, _lib.ptr(mel), lens_keep, _lib.ptr(f0t), _lib.ptr(phase0),
                                                     _lib.ptr(noise), B, S, float(tau), rows, len(names), _lib.stream_ptr()))
        return self._report(names, rows)

    @torch.inference_mode()
    def noise_draws(self, seed, n_frames):
        """(phase0 (1, nh, 1), noise (1, nh, n_frames * up)): the draws `__call__(seeds=[seed])` uses for an utterance of
        n_frames frames (`svc_hift_noise_draws`)."""
        seed = _lib.seeds_host([seed], 1, "HiFT.noise_draws")[0]
        nh, n = self.cfg["nb_harmonics"] + 1, int(n_frames) * self.total_up
        with torch.cuda.device(self.device):
            phase0 = torch.empty(1, nh, 1, device=self.device, dtype=torch.float32)
            noise = torch.empty(1, nh, n, device=self.device, dtype=torch.float32)
            _lib.check(_lib.lib().svc_hift_noise_draws(seed, nh, n, _lib.ptr(phase0), _lib.ptr(noise), _lib.stream_ptr()))
        return phase0, noise

    def close(self):
        if self._h:
            _lib.lib().svc_hift_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
