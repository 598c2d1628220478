"""Residual-shifting diffusion sampler, host side (reference: models/gaussian_diffusion.py:32-66,107-609,
models/respace.py:23-70, models/script_util.py:7-56).

`create_gaussian_diffusion(**yaml.diffusion.params)` returns an object with the reference's sampling
API (`p_sample_loop`, `p_sample_loop_progressive`, `p_sample`, `p_mean_variance`,
`encode_first_stage`, `decode_first_stage`, `prior_sample`, `_scale_input`, `num_timesteps`, ...).
Schedule constants are computed in float64 numpy exactly like the reference; all tensor work is done by
the HIP engine.  When `model` / `first_stage_model` are the engine-backed `UNetModelSwin` /
`VQModelTorch`, `p_sample_loop` runs the whole loop in ONE native call (`rs_sample`).
Per-sample timesteps are honoured as the reference's `_extract_into_tensor` does (gaussian_diffusion.py:92-105): a `t` whose entries
differ runs the per-image elementwise kernel (`rs_axpbypcz_rows`) and a mixed-timestep UNet call; a uniform `t` keeps the scalar calls.
`q_sample` (the forward process, :190-208) is provided; `training_losses` is out of scope.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .autoencoder import VQModelTorch
from .engine import F16, F32, Engine, parse_precision
from .unet import UNetModelSwin, params_version


def get_named_eta_schedule(schedule_name, num_diffusion_timesteps, min_noise_level, etas_end=0.99, kappa=1.0, kwargs=None):
    """sqrt(eta_t), t = 0..T-1 (gaussian_diffusion.py:32-66); only the 'exponential' family is shipped."""
    if schedule_name != "exponential":
        raise ValueError(f"Unknow schedule_name {schedule_name}")
    power = kwargs.get("power", None)
    T = num_diffusion_timesteps
    etas_start = min(min_noise_level / kappa, min_noise_level)
    growth = math.exp(math.log(etas_end / etas_start) / (T - 1))
    exponent = np.linspace(0, 1, T, endpoint=True) ** power * (T - 1)
    return np.power(np.full([T], growth), exponent) * etas_start


def space_timesteps(num_timesteps, sample_timesteps):
    """respace.py:6-18"""
    return set(int((num_timesteps / sample_timesteps) * x) for x in range(sample_timesteps))


class ResShiftDiffusion:
    """Sampling half of GaussianDiffusion + SpacedDiffusion (predict_type 'xstart')."""

    def __init__(self, *, sqrt_etas, kappa, use_timesteps, sf=4, scale_factor=None, normalize_input=True, latent_flag=True,
                 predict_type="xstart"):
        if predict_type != "xstart":
            raise NotImplementedError("engine implements predict_type='xstart' (all shipped configs)")
        self.kappa = kappa
        self.sf = sf
        self.scale_factor = scale_factor
        self.normalize_input = normalize_input
        self.latent_flag = latent_flag
        use = set(use_timesteps)
        self.original_num_steps = len(sqrt_etas)
        self.timestep_map = [i for i in range(len(sqrt_etas)) if i in use]  # respace.py:31-46
        self.sqrt_etas = np.array([sqrt_etas[i] for i in self.timestep_map], dtype=np.float64)
        self.etas = self.sqrt_etas ** 2
        assert (self.etas > 0).all() and (self.etas <= 1).all()
        self.num_timesteps = int(self.etas.shape[0])
        # posterior q(x_{t-1} | x_t, x_0) (gaussian_diffusion.py:149-161)
        self.etas_prev = np.append(0.0, self.etas[:-1])
        self.alpha = self.etas - self.etas_prev
        self.posterior_variance = kappa ** 2 * self.etas_prev / self.etas * self.alpha
        self.posterior_variance_clipped = np.append(self.posterior_variance[1], self.posterior_variance[1:])
        self.posterior_log_variance_clipped = np.log(self.posterior_variance_clipped)
        self.posterior_mean_coef1 = self.etas_prev / self.etas
        self.posterior_mean_coef2 = self.alpha / self.etas
        # precision policy of the engine-backed loop: None -> fp16 under autocast, else fp32
        self.precision_unet = None
        self.precision_encode = None
        self.precision_decode = None
        self._fused: Dict[tuple, tuple] = {}

    # ---- scalar tables handed to the native loop
    def step_tables(self) -> Dict[str, np.ndarray]:
        f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)  # _extract_into_tensor(...).float()
        if self.normalize_input and self.latent_flag:
            inv_std = 1.0 / np.sqrt(f32(self.etas).astype(np.float64) * self.kappa ** 2 + 1)
        elif self.normalize_input:
            inv_std = 1.0 / (f32(self.sqrt_etas).astype(np.float64) * self.kappa * 3 + 1)
        else:
            inv_std = np.ones_like(self.etas)
        return {
            "inv_std": f32(inv_std),
            "coef1": f32(self.posterior_mean_coef1),
            "coef2": f32(self.posterior_mean_coef2),
            "sigma": f32(np.exp(0.5 * f32(self.posterior_log_variance_clipped).astype(np.float64))),
            "tmap": np.asarray(self.timestep_map, dtype=np.int32),
            "prior_scale": np.float32(self.kappa * self.sqrt_etas[-1]),
        }

    def _prec(self, which: Optional[int]) -> int:
        if which is not None:
            return parse_precision(which)
        return F16 if torch.is_autocast_enabled() else F32

    def set_precision(self, unet=None, encode=None, decode=None):
        """unet: 'fp16' | 'fp32' | 'split' (alias 'fp16x3') | list with one entry per timestep t (index = t); encode / decode: one name."""
        self.precision_unet, self.precision_encode, self.precision_decode = unet, encode, decode

    def _unet_precisions(self):
        pu = self.precision_unet
        if isinstance(pu, (list, tuple)):
            assert len(pu) == self.num_timesteps
            return [parse_precision(p) for p in pu]
        return [self._prec(pu)] * self.num_timesteps

    # ---- fused engine (UNet + AE in one native object)
    def _fused_engine(self, model: UNetModelSwin, ae: VQModelTorch) -> Engine:
        key = (id(model), id(ae))
        ver = (params_version(model), params_version(ae))
        ent = self._fused.get(key)
        dev = next(model.parameters()).device
        if ent is None or ent[0].device != dev:
            ent = (Engine(unet_params=model.params, ae_params=ae.params, device=dev), None)
        if ent[1] != ver:
            ent[0].load_state_dicts(unet_sd=model.state_dict(), ae_sd=ae.state_dict())
            ent = (ent[0], ver)
        self._fused[key] = ent
        return ent[0]

    def adopt_engine(self, model: UNetModelSwin, ae: VQModelTorch, engine: Engine):
        """Use an already-loaded engine (e.g. one whose weights arrived by RCCL broadcast) for this model pair.  The module
        shells adopt it too: on ranks > 0 (and after a blob-cache hit) their own parameters were never filled, so
        `model.engine()` / `autoencoder.engine()` - the step-wise API, `model(x, t)`, `encode` / `decode` - must not rebuild an
        engine from those zeros."""
        self._fused[(id(model), id(ae))] = (engine, (params_version(model), params_version(ae)))
        for m in (model, ae):
            m._engine, m._engine_version = engine, params_version(m)

    # ---- per-sample coefficient rows (_extract_into_tensor: the float64 table entry of each sample's t, as float32)
    @staticmethod
    def _t_list(t, B: int):
        """`t` (int, sequence or tensor of step indices) -> one int per sample"""
        if torch.is_tensor(t):
            v = [int(q) for q in t.reshape(-1).tolist()]
        elif isinstance(t, (list, tuple, np.ndarray)):
            v = [int(q) for q in t]
        else:
            v = [int(t)]
        if len(v) == 1:
            v = v * B
        if len(v) != B:
            raise ValueError(f"{len(v)} timesteps for a batch of {B}")
        return v

    def scale_input_coefs(self, ts):
        """per sample: 1 / std of _scale_input (:598-609)"""
        return [float(self.step_tables()["inv_std"][i]) for i in ts]

    def posterior_coefs(self, ts):
        """per sample: (posterior_mean_coef1, posterior_mean_coef2, sqrt(posterior variance) or 0 at t = 0) (:210-221,358-364)"""
        tab = self.step_tables()
        return ([float(tab["coef1"][i]) for i in ts], [float(tab["coef2"][i]) for i in ts],
                [float(tab["sigma"][i]) if i != 0 else 0.0 for i in ts])

    def q_sample_coefs(self, ts):
        """per sample: (1 - eta_t, eta_t, kappa * sqrt(eta_t)) of q_sample (:190-208)"""
        f32 = lambda v: float(np.float32(v))
        return ([f32(1.0 - self.etas[i]) for i in ts], [f32(self.etas[i]) for i in ts], [f32(self.kappa * self.sqrt_etas[i]) for i in ts])

    @staticmethod
    def _rows(x, z, n, a, b, c, engine=None):
        """per-image a[i]*x[i] + b[i]*z[i] + c[i]*n[i] on the engine's kernel (rs_axpbypcz_rows); no CPU path, as _axpbypcz"""
        if engine is None or not x.is_cuda:
            raise RuntimeError("step-wise sampling needs the HIP engine (engine-backed UNetModelSwin on a GPU); no CPU fallback")
        return engine.axpbypcz_rows(x, z, n, a, b, c).to(x.dtype)

    def _any_engine(self):
        for eng, _ in self._fused.values():
            return eng
        raise RuntimeError("q_sample needs the HIP engine: pass engine= or build the sampler's models first; no CPU fallback")

    # ---- reference API
    @staticmethod
    def _axpbypcz(x, z, n, a, b, c, engine=None):
        """a*x + b*z + c*n on the engine's elementwise kernel.  There is deliberately no torch/CPU arithmetic path: the
        step-wise API needs the engine-backed UNetModelSwin (it owns the device kernels)."""
        if engine is None or not x.is_cuda:
            raise RuntimeError("step-wise sampling needs the HIP engine (engine-backed UNetModelSwin on a GPU); no CPU fallback")
        return engine.axpbypcz(x, z, n, a, b, c).to(x.dtype)

    def _scale_input(self, inputs, t, engine=None):
        ts = self._t_list(t, inputs.shape[0])
        if len(set(ts)) > 1:
            return self._rows(inputs, None, None, self.scale_input_coefs(ts), [0.0] * len(ts), [0.0] * len(ts), engine)
        tab = self.step_tables()["inv_std"]
        ti = ts[0]
        return self._axpbypcz(inputs, None, None, float(tab[ti]), 0.0, 0.0, engine)

    def q_sample(self, x_start, y, t, noise=None, engine=None):
        """gaussian_diffusion.py:190-208: x_t = (1 - eta_t) x_0 + eta_t y + kappa sqrt(eta_t) noise, per sample"""
        if noise is None:
            noise = torch.randn_like(x_start)
        engine = engine if engine is not None else self._any_engine()
        ts = self._t_list(t, x_start.shape[0])
        a, b, c = self.q_sample_coefs(ts)
        if len(set(ts)) > 1:
            return self._rows(x_start, y, noise, a, b, c, engine)
        return self._axpbypcz(x_start, y, noise, a[0], b[0], c[0], engine)

    def prior_sample(self, y, noise=None, engine=None):
        if noise is None:
            noise = torch.randn_like(y)
        return self._axpbypcz(y, None, noise, 1.0, 0.0, float(np.float32(self.kappa * self.sqrt_etas[-1])), engine)

    def q_posterior_mean_variance(self, x_start, x_t, t, engine=None):
        ts = self._t_list(t, x_t.shape[0])
        if len(set(ts)) > 1:
            c1, c2, _ = self.posterior_coefs(ts)
            mean = self._rows(x_t, x_start, None, c1, c2, [0.0] * len(ts), engine)
            per = lambda arr: torch.tensor([float(np.float32(arr[i])) for i in ts], dtype=torch.float32,
                                           device=x_t.device).view(-1, *[1] * (x_t.dim() - 1)).expand_as(x_t).clone()
            return mean, per(self.posterior_variance), per(self.posterior_log_variance_clipped)
        ti = ts[0]
        tab = self.step_tables()
        mean = self._axpbypcz(x_t, x_start, None, float(tab["coef1"][ti]), float(tab["coef2"][ti]), 0.0, engine)
        var = torch.full_like(x_t, float(np.float32(self.posterior_variance[ti])))
        logvar = torch.full_like(x_t, float(np.float32(self.posterior_log_variance_clipped[ti])))
        return mean, var, logvar

    def encode_first_stage(self, y, first_stage_model, up_sample=False):
        """gaussian_diffusion.py:500-515"""
        if first_stage_model is None:
            if up_sample and self.sf != 1:
                raise RuntimeError("bicubic upsampling needs an engine; pass the autoencoder")
            return y
        eng = first_stage_model.engine()
        if up_sample and self.sf != 1:
            y = eng.bicubic(y, self.sf)
        z = first_stage_model.encode(y, prec=self._prec(self.precision_encode))
        return _lib.window_copy(z, scale=self.scale_factor) if self.scale_factor != 1.0 else z   # (one fp32 multiply on the device)

    def decode_first_stage(self, z_sample, first_stage_model=None, consistencydecoder=None):
        """gaussian_diffusion.py:474-498"""
        if consistencydecoder is not None:
            raise NotImplementedError("consistency decoder is out of scope")
        if first_stage_model is None:
            return z_sample
        if self.scale_factor != 1.0:
            z_sample = _lib.window_copy(z_sample, scale=1.0 / self.scale_factor)
        return first_stage_model.decode(z_sample, prec=self._prec(self.precision_decode))

    def p_mean_variance(self, model, x_t, y, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """gaussian_diffusion.py:234-307 (START_X).  `t`: [B] step indices, equal or not."""
        model_kwargs = model_kwargs or {}
        tl = self._t_list(t, x_t.shape[0])
        precs = {self._unet_precisions()[i] for i in tl}
        if len(precs) > 1:
            raise NotImplementedError("a batch whose steps run the UNet at different precisions (per-step mixed precision policy)")
        prec = precs.pop()
        ts = [self.timestep_map[i] for i in tl]  # _WrappedModel (respace.py:67-70)
        if not isinstance(model, UNetModelSwin):
            raise NotImplementedError("p_mean_variance drives the engine-backed UNetModelSwin only")
        eng = model.engine()
        ti = tl[0] if len(set(tl)) == 1 else tl
        pred = model(self._scale_input(x_t, ti, eng), ts, prec=prec, **model_kwargs)
        if denoised_fn is not None:
            pred = denoised_fn(pred)
        if clip_denoised:
            pred = pred.clamp(-1, 1)
        mean, var, logvar = self.q_posterior_mean_variance(pred, x_t, ti, eng)
        return {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": pred}

    def p_sample(self, model, x, y, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, noise_repeat=False, noise=None):
        """gaussian_diffusion.py:332-365; `noise` may be injected for parity runs (draws randn_like otherwise)."""
        out = self.p_mean_variance(model, x, y, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs)
        if noise is None:
            noise = torch.randn_like(x)
        if noise_repeat:
            noise = noise[0,].repeat(x.shape[0], 1, 1, 1)
        tl = self._t_list(t, x.shape[0])
        eng = model.engine() if isinstance(model, UNetModelSwin) else None
        if len(set(tl)) > 1:
            sig = self.posterior_coefs(tl)[2]   # (nonzero_mask: no noise at t = 0)
            sample = self._rows(out["mean"], None, noise, [1.0] * len(tl), [0.0] * len(tl), sig, eng)
            return {"sample": sample, "pred_xstart": out["pred_xstart"], "mean": out["mean"]}
        ti = tl[0]
        sigma = float(self.step_tables()["sigma"][ti]) if ti != 0 else 0.0
        sample = self._axpbypcz(out["mean"], None, noise, 1.0, 0.0, sigma, eng)
        return {"sample": sample, "pred_xstart": out["pred_xstart"], "mean": out["mean"]}

    @staticmethod
    def _seed_keys(seeds, B: int, noise, step_noises, noise_repeat):
        """seeds= of p_sample_loop -> [(seed, stream)] per image"""
        if noise is not None or step_noises is not None or noise_repeat:
            raise ValueError("seeds= names every draw: it excludes noise, step_noises and noise_repeat")
        keys = [tuple(int(v) for v in k) if isinstance(k, (tuple, list)) else (int(k), 0) for k in seeds]
        if len(keys) != B:
            raise ValueError(f"seeds: {B} images but {len(keys)} seeds")
        return keys

    def p_sample_loop_progressive(self, y, model, first_stage_model=None, noise=None, noise_repeat=False, clip_denoised=True,
                                  denoised_fn=None, model_kwargs=None, device=None, progress=False, step_noises=None, seeds=None):
        """gaussian_diffusion.py:421-472: generator of per-step dicts {"sample","pred_xstart","mean"}.  `seeds`: see p_sample_loop (every
        draw is the seeded definition's, one rs_noise_fill call per draw)."""
        z_y = self.encode_first_stage(y, first_stage_model, up_sample=True)
        if seeds is not None:
            keys = self._seed_keys(seeds, z_y.shape[0], noise, step_noises, noise_repeat)
            eng = model.engine() if isinstance(model, UNetModelSwin) else self._any_engine()
            fill = lambda k: eng.noise_fill(keys, [k] * len(keys), tuple(z_y.shape[1:]))
            noise, step_noises = fill(0), [fill(k) for k in range(1, self.num_timesteps + 1)]
        if noise is None:
            noise = torch.randn_like(z_y)
        if noise_repeat:
            noise = noise[0,].repeat(z_y.shape[0], 1, 1, 1)
        z_sample = self.prior_sample(z_y, noise, model.engine() if isinstance(model, UNetModelSwin) else None)
        for k, i in enumerate(list(range(self.num_timesteps))[::-1]):
            t = torch.tensor([i] * y.shape[0])   # (kept on the host: the shells read the step index from it - a device tensor would cost a sync per step)
            out = self.p_sample(model, z_sample, z_y, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                model_kwargs=model_kwargs, noise_repeat=noise_repeat,
                                noise=None if step_noises is None else step_noises[k])
            yield out
            z_sample = out["sample"]

    def p_sample_loop(self, y, model, first_stage_model=None, consistencydecoder=None, noise=None, noise_repeat=False,
                      clip_denoised=True, denoised_fn=None, model_kwargs=None, device=None, progress=False, step_noises=None,
                      return_aux=False, seeds=None):
        """gaussian_diffusion.py:367-419.  Fast path: one native `rs_sample` call for the whole loop.
        `seeds`: one per image - an int (stream 0) or a (seed, stream) pair.  Image b then gets draws 0 .. steps of its key
        whatever the batch, the slot or the process: no torch.randn, no noise tensor (fast path: `rs_sample_seeded`, the normals are made
        in the kernels that consume them).  Mutually exclusive with noise / step_noises / noise_repeat."""
        fused_ok = (isinstance(model, UNetModelSwin) and isinstance(first_stage_model, VQModelTorch) and consistencydecoder is None
                    and denoised_fn is None and not clip_denoised)
        if not fused_ok:
            final = None
            for sample in self.p_sample_loop_progressive(y, model, first_stage_model=first_stage_model, noise=noise,
                                                         noise_repeat=noise_repeat, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                         model_kwargs=model_kwargs, device=device, progress=progress,
                                                         step_noises=step_noises, seeds=seeds):
                final = sample["sample"]
            return self.decode_first_stage(final, first_stage_model=first_stage_model, consistencydecoder=consistencydecoder)
        eng = self._fused_engine(model, first_stage_model)
        B, _, h, w = y.shape
        if seeds is not None:   # nothing is drawn: the kernels make the normals of each key
            noise_all, keys = None, self._seed_keys(seeds, B, noise, step_noises, noise_repeat)
        else:
            zshape = eng.latent_shape(B, h, w, self.sf)
            # RNG draws in the reference's order: prior noise (:446), then one randn_like per step (:358)
            draws = []
            for k in range(self.num_timesteps + 1):
                if k == 0 and noise is not None:
                    n = noise
                elif k > 0 and step_noises is not None:
                    n = step_noises[k - 1]
                else:
                    n = torch.randn(zshape, device=y.device, dtype=torch.float32)
                n = n.to(y.device, torch.float32)
                if noise_repeat:
                    n = n[0,].repeat(B, 1, 1, 1)
                draws.append(n)
            noise_all, keys = torch.stack(draws, 0), None
        mask = (model_kwargs or {}).get("mask", None)
        lq = (model_kwargs or {}).get("lq", None)
        if lq is not None and lq.data_ptr() != y.data_ptr() and not torch.equal(lq, y):
            raise NotImplementedError("fused loop conditions the UNet on y itself (sampler.py:140-148)")
        return eng.sample(y, noise_all, self.step_tables(), sf=self.sf, scale_factor=self.scale_factor, mask=mask,
                          prec_unet=self._unet_precisions(), prec_encode=self._prec(self.precision_encode),
                          prec_decode=self._prec(self.precision_decode), return_aux=return_aux, keys=keys)


def create_gaussian_diffusion(*, normalize_input, schedule_name, sf=4, min_noise_level=0.01, steps=1000, kappa=1, etas_end=0.99,
                              schedule_kwargs=None, weighted_mse=False, predict_type="xstart", timestep_respacing=None,
                              scale_factor=None, latent_flag=True):
    """models/script_util.py:7-56 — same keyword signature; returns the engine-backed sampler."""
    sqrt_etas = get_named_eta_schedule(schedule_name, num_diffusion_timesteps=steps, min_noise_level=min_noise_level,
                                       etas_end=etas_end, kappa=kappa, kwargs=schedule_kwargs)
    if timestep_respacing is None:
        timestep_respacing = steps
    else:
        assert isinstance(timestep_respacing, int)
    return ResShiftDiffusion(sqrt_etas=sqrt_etas, kappa=kappa, use_timesteps=space_timesteps(steps, timestep_respacing), sf=sf,
                             scale_factor=1.0 if scale_factor is None else scale_factor, normalize_input=normalize_input,
                             latent_flag=latent_flag, predict_type=predict_type)
