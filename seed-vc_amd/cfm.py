"""Host-side mirror of the reference's sampler / estimator interface over the C ABI.

`CFM.inference(mu, x_lens, prompt, style, f0, n_timesteps, temperature=1.0, inference_cfg_rate=0.5)`
keeps the reference signature (modules/flow_matching.py:30-31; v2: modules/v2/cfm.py:16-25), so a
driver that calls `model.cfm.inference(...)` (inference.py:483-505, seed_vc_wrapper.py:575-603) runs
unchanged.  Differences that are additions, not changes: `z=` lets the caller supply the noise
(otherwise torch.randn like the reference), `seeds=` gives one 64-bit seed per utterance and the noise is drawn on the
device inside the sampler (`svc_cfm_sample_seeded`; `CFM.noise_draws` returns the same tensor), and B > 1 is accepted and means B independent B=1 runs
(the reference sampler raises for B > 1).
"""
import ctypes as C

import torch

from . import _lib
from .specs import dit_config


def _cfg_struct(cfg):
    c = _lib.DitConfig()
    c.version = cfg["version"]
    c.hidden_dim, c.num_heads, c.depth = cfg["D"], cfg["H"], cfg["L"]
    c.in_channels, c.content_dim, c.style_dim = cfg["C"], cfg["Dc"], cfg["style_dim"]
    c.final_layer_type = 1 if cfg["head"] == "wavenet" else 0
    c.time_as_token, c.style_as_token = int(cfg["time_as_token"]), int(cfg["style_as_token"])
    c.uvit_skip_connection, c.long_skip_connection = int(cfg["uvit"]), int(cfg["long_skip"])
    c.style_condition = int(cfg["style_condition"])
    c.wn_hidden_dim = cfg.get("wn_dim", 0)
    c.wn_num_layers = cfg.get("wn_layers", 0)
    c.wn_kernel_size = cfg.get("wn_kernel", 0)
    c.wn_dilation_rate = cfg.get("wn_dilation", 1)
    return c


def sampler_setting(entry, what="settings"):
    """One utterance's sampler settings -> (n_timesteps, (rate_a, rate_b), temperature, random_voice).  entry: a dict with
    the keys n_timesteps, inference_cfg_rate and optionally temperature (1.0), random_voice (False), or a tuple in that
    order.  A rate is a float (v2: both rates) or a pair, as `CFM.inference` takes it."""
    if isinstance(entry, dict):
        unknown = set(entry) - {"n_timesteps", "inference_cfg_rate", "temperature", "random_voice"}
        if unknown or "n_timesteps" not in entry or "inference_cfg_rate" not in entry:
            raise ValueError(f"{what}: an entry needs n_timesteps and inference_cfg_rate (optional: temperature, random_voice), "
                             f"got the keys {sorted(entry)}")
        entry = (entry["n_timesteps"], entry["inference_cfg_rate"], entry.get("temperature", 1.0), entry.get("random_voice", False))
    if not isinstance(entry, (list, tuple)) or not 2 <= len(entry) <= 4:
        raise ValueError(f"{what}: an entry is a dict or (n_timesteps, inference_cfg_rate[, temperature[, random_voice]]), got {entry!r}")
    steps, rate = entry[0], entry[1]
    temperature = entry[2] if len(entry) > 2 else 1.0
    random_voice = entry[3] if len(entry) > 3 else False
    if isinstance(rate, (list, tuple)):
        if len(rate) != 2:
            raise ValueError(f"{what}: a pair of rates has two entries, got {rate!r}")
        rate = (float(rate[0]), float(rate[1]))
    else:
        rate = (float(rate), float(rate))
    return int(steps), rate, float(temperature), bool(random_voice)


def _rows_struct(settings, B, what):
    """settings (B entries of `sampler_setting`) -> the HOST svc_cfm_row_t array."""
    settings = list(settings)
    if len(settings) != B:
        raise ValueError(f"{what}: {len(settings)} settings for {B} utterances")
    rows = (_lib.CfmRow * B)()
    for r, e in zip(rows, settings):
        r.n_timesteps, (r.cfg_rate[0], r.cfg_rate[1]), r.temperature, rv = sampler_setting(e, what)
        r.random_voice = int(rv)
    return rows


PRECISIONS = {1: 1, 2: 2, "fp16": 1, "fp16x3": 2}


def dit_precision(precision):
    """1 | "fp16" (fp16 GEMM / attention operands) or 2 | "fp16x3" (split precision, fp32-level results) -> 1 | 2
    (`svc_dit_create_ex`, include/seedvc_hip.h).  Anything else raises before a handle or a weight is touched."""
    if isinstance(precision, bool) or not isinstance(precision, (int, str)) or precision not in PRECISIONS:
        raise ValueError(f"DiT precision must be 1 / 'fp16' or 2 / 'fp16x3', got {precision!r}")
    return PRECISIONS[precision]


class Estimator:
    """Packed DiT on one device (mirror of `CFM.estimator`).  precision: see `dit_precision`; fixed for the handle's life."""

    def __init__(self, cfg, state_dict, device="cuda:0", precision=1):
        self._h = C.c_void_p()
        self._precision = dit_precision(precision)
        self.cfg = cfg
        self.device = torch.device(device)
        self.in_channels = cfg["C"]
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            cs = _cfg_struct(cfg)
            _lib.check(_lib.lib().svc_dit_create_ex(C.byref(cs), descs, n, self._precision, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    @property
    def precision(self):
        """1 (fp16 operands) or 2 (fp16x3)."""
        return self._precision

    def setup_caches(self, max_batch_size=1, max_seq_length=8192):
        """No-op kept for call compatibility (inference.py:90): RoPE table and skip lists are built at pack time."""
        return None

    def set_microbatch(self, n):
        _lib.check(_lib.lib().svc_dit_set_microbatch(self._h, int(n)))

    def set_fused_min_rows(self, rows):
        """Token rows per launch from which the transformer layers use the fused row-panel kernel (-1: default)."""
        _lib.check(_lib.lib().svc_dit_set_fused_min_rows(self._h, C.c_long(int(rows))))

    def set_fused_seams(self, mask):
        """Sampler seams inside the fused row-panel launches: bit 0 merge linear + token rows, bit 1 mlp head (default 3)."""
        _lib.check(_lib.lib().svc_dit_set_fused_seams(self._h, int(mask)))

    def set_graphs(self, on):
        """hipGraph capture / replay of the sampler's Euler loop (off by default; bit-identical to eager launches)."""
        _lib.check(_lib.lib().svc_dit_set_graphs(self._h, int(bool(on))))

    @property
    def fused_available(self):
        return bool(_lib.lib().svc_dit_fused_available(self._h))

    def __call__(self, x, prompt_x, x_lens, t, style, cond, mask_content=False):
        """estimator(x, prompt_x, x_lens, t, style, mu) -> (N, C, T); reference: diffusion_transformer.py:486."""
        N, Cc, T = x.shape
        with torch.cuda.device(self.device):
            x, prompt_x, style, cond = (_lib.f32c(a, self.device) for a in (x, prompt_x, style, cond))
            out = torch.empty_like(x)
            tval = float(t.reshape(-1)[0]) if torch.is_tensor(t) else float(t)
            lens = None
            if x_lens is not None:
                xl = _lib.int_list(x_lens)
                if len(xl) == 1 and N > 1:
                    xl = xl * N
                lens = _lib.i64_host(xl)
            _lib.check(_lib.lib().svc_dit_forward(self._h, N, T, _lib.ptr(x), _lib.ptr(prompt_x), lens,
                                                  C.c_float(tval), _lib.ptr(style), _lib.ptr(cond), _lib.ptr(out),
                                                  _lib.stream_ptr()))
        return out

    def close(self):
        if self._h:
            _lib.lib().svc_dit_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CFM:
    """Mirror of modules.flow_matching.CFM / modules.v2.cfm.CFM for inference."""

    def __init__(self, cfg, state_dict, device="cuda:0", precision=1):
        self.cfg = cfg
        self.estimator = Estimator(cfg, state_dict, device, precision)
        self.in_channels = cfg["C"]
        self.device = self.estimator.device

    @classmethod
    def from_preset(cls, name, state_dict, device="cuda:0", **overrides):
        return cls(dit_config(name, **overrides), state_dict, device)

    @property
    def precision(self):
        """1 (fp16 operands) or 2 (fp16x3): the estimator's (`dit_precision`)."""
        return self.estimator.precision

    @torch.inference_mode()
    def inference(self, mu, x_lens, prompt, style, f0=None, n_timesteps=10, temperature=1.0,
                  inference_cfg_rate=0.5, random_voice=False, z=None, prompt_lens=None, seeds=None):
        """seeds: B integers in [0, 2^64) (list or tensor), exclusive with z: utterance b starts from the draws of seeds[b], a
        pure function of (seed, channel, frame) -- the same whatever its row, T and its neighbours (include/seedvc_hip.h)."""
        if seeds is not None and z is not None:
            raise ValueError("CFM.inference: give seeds or z, not both")
        seeds_keep = _lib.seeds_host(seeds, mu.size(0), "CFM.inference") if seeds is not None else None
        if self.cfg["version"] == 2 and not isinstance(f0, (type(None), torch.Tensor)):
            # v2 call form: inference(mu, x_lens, prompt, style, n_timesteps, temperature, inference_cfg_rate, ...)
            n_timesteps, f0 = f0, None
        B, T = mu.size(0), mu.size(1)
        dev = self.device
        with torch.cuda.device(dev):
            mu, prompt, style = (_lib.f32c(a, dev) for a in (mu, prompt, style))
            if seeds is None:
                if z is None:
                    z = torch.randn([B, self.in_channels, T], device=dev)      # flow_matching.py:50
                z = _lib.f32c(z, dev)
            out = torch.empty(B, self.in_channels, T, device=dev, dtype=torch.float32)
            a = _lib.CfmArgs()
            a.B, a.T, a.P = B, T, prompt.size(-1)
            a.mu, a.prompt, a.style, a.out = (t.data_ptr() for t in (mu, prompt, style, out))
            a.z = z.data_ptr() if z is not None else None
            xl = None
            if x_lens is not None:
                xl = _lib.int_list(x_lens)
                if len(xl) == 1 and B > 1:
                    xl = xl * B
            lens_keep = _lib.i64_host(xl)
            plens_keep = _lib.i64_host(prompt_lens)
            a.x_lens = lens_keep
            a.prompt_lens = plens_keep
            a.n_timesteps = int(n_timesteps)
            a.temperature = float(temperature)
            if isinstance(inference_cfg_rate, (list, tuple)):
                a.cfg_rate[0], a.cfg_rate[1] = float(inference_cfg_rate[0]), float(inference_cfg_rate[1])
            else:
                a.cfg_rate[0], a.cfg_rate[1] = float(inference_cfg_rate), float(inference_cfg_rate)
            a.random_voice = int(bool(random_voice))
            if seeds_keep is not None:
                _lib.check(_lib.lib().svc_cfm_sample_seeded(self.estimator._h, C.byref(a), seeds_keep, _lib.stream_ptr()))
            else:
                _lib.check(_lib.lib().svc_cfm_sample(self.estimator._h, C.byref(a), _lib.stream_ptr()))
        return out

    def rows_plan(self, settings):
        """The partition `inference_rows` uses for these settings (`svc_cfm_rows_plan`; needs no GPU) ->
        (class_of, n_streams): class_of[b] = class of utterance b, classes numbered by first appearance; n_streams[c] =
        guidance streams (estimator evaluations per step) of class c.  Two utterances share a class, and with it every
        launch, when they have the same n_timesteps and the same guidance structure (include/seedvc_hip.h)."""
        settings = list(settings)
        B = len(settings)
        rows = _rows_struct(settings, B, "CFM.rows_plan")
        class_of, n_streams = (C.c_int32 * max(B, 1))(), (C.c_int32 * max(B, 1))()
        n = _lib.lib().svc_cfm_rows_plan(int(self.cfg["version"]), rows, B, class_of, n_streams)
        if n < 0:
            raise ValueError(_lib.lib().svc_last_error().decode())
        return list(class_of[:B]), list(n_streams[:n])

    @torch.inference_mode()
    def inference_rows(self, mu, x_lens, prompt, style, settings, z=None, prompt_lens=None, seeds=None):
        """`inference` with the steps, the guidance rate(s), the temperature and random_voice of every utterance taken from
        settings[b] (`sampler_setting`: a dict or (n_timesteps, inference_cfg_rate, temperature=1.0, random_voice=False)) in
        ONE call (`svc_cfm_sample_rows`).  Utterance b is the B = 1 run `inference(..., *settings[b])` on its own inputs;
        utterances of one class (`rows_plan`) share every launch whatever their rates and temperatures.  z / seeds as
        `inference` (neither: torch.randn)."""
        if seeds is not None and z is not None:
            raise ValueError("CFM.inference_rows: give seeds or z, not both")
        B, T = mu.size(0), mu.size(1)
        seeds_keep = _lib.seeds_host(seeds, B, "CFM.inference_rows") if seeds is not None else None
        rows = _rows_struct(settings, B, "CFM.inference_rows")
        dev = self.device
        with torch.cuda.device(dev):
            mu, prompt, style = (_lib.f32c(a, dev) for a in (mu, prompt, style))
            if seeds is None:
                if z is None:
                    z = torch.randn([B, self.in_channels, T], device=dev)
                z = _lib.f32c(z, dev)
            out = torch.empty(B, self.in_channels, T, device=dev, dtype=torch.float32)
            a = _lib.CfmArgs()
            a.B, a.T, a.P = B, T, prompt.size(-1)
            a.mu, a.prompt, a.style, a.out = (t.data_ptr() for t in (mu, prompt, style, out))
            a.z = z.data_ptr() if z is not None else None
            xl = None
            if x_lens is not None:
                xl = _lib.int_list(x_lens)
                if len(xl) == 1 and B > 1:
                    xl = xl * B
            lens_keep = _lib.i64_host(xl)
            plens_keep = _lib.i64_host(prompt_lens)
            a.x_lens = lens_keep
            a.prompt_lens = plens_keep
            _lib.check(_lib.lib().svc_cfm_sample_rows(self.estimator._h, C.byref(a), rows, seeds_keep, _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def noise_draws(self, seed, T):
        """(1, C, T): the noise `inference(seeds=[seed])` starts an utterance of T frames from (`svc_cfm_noise_draws`)."""
        seed = _lib.seeds_host([seed], 1, "CFM.noise_draws")[0]
        with torch.cuda.device(self.device):
            z = torch.empty(1, self.in_channels, int(T), device=self.device, dtype=torch.float32)
            _lib.check(_lib.lib().svc_cfm_noise_draws(seed, self.in_channels, int(T), _lib.ptr(z), _lib.stream_ptr()))
        return z
