"""Continuous batching over a built `ResShiftSampler`: images are admitted at every step and retired at every step.

In ResShift every image carries its own state (x_t, its LR conditioning, its mask, its noise draws) and nothing in the network mixes
images (GroupNorm is per sample, attention per window), so one UNet call may hold images at different steps.  `ContinuousSampler`
keeps a dense pool of active images and, per `step()`:

  1. admits waiting images (up to `max_batch` active) as ONE `rs_sample_begin` batch (bicubic + encode + prior_sample);
  2. runs ONE `rs_sample_step` over every active image, each at its own step index (per-image FiLM rows and elementwise coefficients
     inside the engine; a pool whose images are all at one step runs the launches of `rs_sample`'s step);
  3. retires the images that just finished t = 0 as ONE `rs_sample_end` batch (decode) and compacts the pool;
  4. crops and clamps each result as `ResShiftSampler.sample_func` does.

Same engine, precision policy and `padding_offset` as the sampler it wraps.  One LR size per instance: images of any size, cut into
tiles that share such pools, are `tilepool.TilePool`'s business (it drives one ContinuousSampler per padded tile shape).  Out of scope:
per-step mixed precision policies, `noise_repeat` (it is defined by a fixed batch, which a pool does not have - in either noise mode),
pixel-space models (no autoencoder).

`seeded=True`: a request is named by a seed and its noise is generated inside the engine's kernels from
(seed, stream, draw index, element index) - no torch.randn at submit time, no draws in the pool, no per-step gather.  What a request
gets no longer depends on the requests before it, on its slot or on the process that serves it.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Dict, List, Optional

import torch

from . import _lib, sharding


def request_seed(base_seed: int, index: int) -> int:
    """The default seed of request `index` under a sampler seeded with `base_seed`: (base_seed * 2^32 + index) mod 2^64 - distinct for
    every index below 2^32, and a pure function of the two numbers (no generator state)."""
    return ((int(base_seed) << 32) + int(index)) % 2 ** 64


def check_sampler(sampler, max_batch, who: str = "ContinuousSampler"):
    """what a pool of images at different steps asks of the sampler it wraps; returns the per-step UNet precisions"""
    if getattr(sampler, "autoencoder", None) is None:
        raise NotImplementedError(f"{who} samples in the VQ latent space: the sampler needs an autoencoder")
    if max_batch is not None and not 1 <= int(max_batch) <= _lib.RS_MAX_ROWS:
        raise ValueError(f"max_batch must be 1 .. {_lib.RS_MAX_ROWS} (RS_MAX_ROWS), got {max_batch}")
    precs = sampler.base_diffusion._unet_precisions()
    if len(set(precs)) > 1:
        raise NotImplementedError(f"{who} needs one UNet precision for every step; this policy varies it by step (mixedK)")
    return precs


class ContinuousSampler:
    def __init__(self, sampler, max_batch: int = 32, keep_aux: bool = False, seeded: bool = False):
        """`keep_aux`: also keep each finished image's final latent and VQ indices in `self.aux[id]` ({"z_final", "indices"}, as
        p_sample_loop's return_aux).  `seeded`: requests carry a (seed, stream) key instead of noise tensors (module docstring)."""
        precs = check_sampler(sampler, max_batch)
        d = sampler.base_diffusion
        self.sampler, self.diffusion, self.engine = sampler, d, sampler.engine
        self.max_batch = int(max_batch)
        self.tables = d.step_tables()
        self.steps = int(d.num_timesteps)
        self.prec_unet = precs[0]
        self.prec_encode, self.prec_decode = d._prec(d.precision_encode), d._prec(d.precision_decode)
        self.sf, self.scale_factor, self.offset = int(d.sf), float(d.scale_factor), int(sampler.padding_offset)
        self.cond_mask = bool(sampler.configs["model"]["params"].get("cond_mask", False))
        self.device = getattr(sampler, "device", None) or torch.device("cuda", torch.cuda.current_device())
        # every step index of the schedule is used: build their FiLM rows now, so that no step pays film_row's synchronise
        self.engine.film_prewarm([int(v) for v in self.tables["tmap"]])
        self._waiting: deque = deque()   # (id, y [3,hp,wp], mask [1,hp,wp] | None, draws [steps+1,Cz,hz,wz])
        self._next_id = 0
        self.lr_size = None              # (h, w) of the first request: the one LR size of this instance
        self._pad = (0, 0)
        # the slot pool: active images are slots 0 .. n-1 (dense; compacted on retire)
        self._n = 0
        self._ids: List[int] = []
        self._t: List[int] = []          # step index of each slot's next step (steps-1 .. 0)
        self._X = self._Y = self._M = self._N = None
        self.seeded = bool(seeded)
        self._keys: List[tuple] = []     # seeded: (seed, stream) of each slot (no _N then)
        self.keep_aux = bool(keep_aux)
        self.aux: Dict[int, Dict[str, torch.Tensor]] = {}

    # ------------------------------------------------------------------ requests
    def submit(self, lq, mask=None, noise=None, step_noises=None, noise_repeat=False, seed=None, stream=0) -> List[int]:
        """Queue LR images lq [n,3,h,w] (or [3,h,w]) in [-1,1]; returns one id per image.  `noise` [n,Cz,hz,wz] and `step_noises`
        (steps tensors [n,Cz,hz,wz], in loop order) inject the draws; otherwise they are drawn now, in the reference's order (prior
        noise, then one per step: gaussian_diffusion.py:446,358).
        Seeded mode: `seed` (an int for every image of the call, or one per image; default request_seed(sampler.seed, id)) and `stream`
        name each image's noise; tensors are rejected.  `noise_repeat` is unsupported in both modes."""
        if noise_repeat:
            raise NotImplementedError("noise_repeat shares one draw across a batch; continuous batching has no fixed batch")
        if self.seeded and (noise is not None or step_noises is not None):
            raise ValueError("a seeded ContinuousSampler generates its noise from seeds: noise / step_noises tensors are not accepted")
        if not self.seeded and (seed is not None or stream != 0):
            raise ValueError("seed= / stream= need ContinuousSampler(..., seeded=True)")
        if lq.dim() == 3:
            lq = lq.unsqueeze(0)
            mask = mask.unsqueeze(0) if mask is not None and mask.dim() == 3 else mask
        n, _, h, w = lq.shape
        if self.lr_size is None:
            self.lr_size = (h, w)
            self._pad = ((math.ceil(h / self.offset)) * self.offset - h, (math.ceil(w / self.offset)) * self.offset - w)
        elif (h, w) != self.lr_size:
            raise ValueError(f"this ContinuousSampler serves {self.lr_size[0]}x{self.lr_size[1]} LR images; got {h}x{w} (one LR size per instance)")
        if self.cond_mask and mask is None:
            raise ValueError("this model is conditioned on a mask (cond_mask): submit(lq, mask=...)")
        lq = lq.to(self.device, torch.float32)
        mask = mask.to(self.device, torch.float32) if (mask is not None and self.cond_mask) else None
        if self._pad != (0, 0):   # sample_func's reflect padding (sampler.py:130-138), the mask alike
            lq = sharding.reflect_pad(lq, *self._pad)
            mask = sharding.reflect_pad(mask, *self._pad) if mask is not None else None
        if self.seeded:   # per-request payload: the (seed, stream) key
            seeds = [int(v) for v in seed] if isinstance(seed, (list, tuple)) else [seed] * n
            if len(seeds) != n:
                raise ValueError(f"seed: {n} images but {len(seeds)} seeds")
            base = getattr(self.sampler, "seed", 0)
            draws = [(int(sd if sd is not None else request_seed(base, self._next_id + i)) % 2 ** 64, int(stream)) for i, sd in enumerate(seeds)]
        else:             # ... or its row of the stacked draws
            zs = self.engine.latent_shape(n, lq.shape[2], lq.shape[3], self.sf)
            if noise is None:
                noise = torch.randn(zs, device=self.device, dtype=torch.float32)
            if step_noises is None:
                step_noises = [torch.randn(zs, device=self.device, dtype=torch.float32) for _ in range(self.steps)]
            if len(step_noises) != self.steps:
                raise ValueError(f"step_noises: {self.steps} draws expected, got {len(step_noises)}")
            draws = torch.stack([noise.to(self.device, torch.float32)] + [s.to(self.device, torch.float32) for s in step_noises], 1)
            if tuple(draws.shape) != (n, self.steps + 1) + tuple(zs[1:]):
                raise ValueError(f"noise draws must be [{n},{zs[1]},{zs[2]},{zs[3]}] each, got {tuple(draws.shape)}")
        ids = []
        for i in range(n):
            self._waiting.append((self._next_id, lq[i], mask[i] if mask is not None else None, draws[i]))
            ids.append(self._next_id)
            self._next_id += 1
        return ids

    def pending(self) -> int:
        """images waiting or in flight"""
        return len(self._waiting) + self._n

    @property
    def active(self) -> int:
        return self._n

    # ------------------------------------------------------------------ scheduling
    def _alloc(self, y, m, draws):
        B = self.max_batch
        zs = tuple(self.engine.latent_shape(1, y.shape[-2], y.shape[-1], self.sf))[1:] if self.seeded else tuple(draws.shape[1:])
        self._X = torch.empty((B,) + zs, device=self.device, dtype=torch.float32)
        self._Y = torch.empty((B,) + tuple(y.shape), device=self.device, dtype=torch.float32)
        self._M = torch.empty((B,) + tuple(m.shape), device=self.device, dtype=torch.float32) if m is not None else None
        if not self.seeded:   # (seeded: the draws are never stored)
            self._N = torch.empty((B,) + tuple(draws.shape), device=self.device, dtype=torch.float32)

    def _admit(self):
        m = min(len(self._waiting), self.max_batch - self._n)
        if m <= 0:
            return
        reqs = [self._waiting.popleft() for _ in range(m)]
        if self._X is None:
            self._alloc(reqs[0][1], reqs[0][2], reqs[0][3])
        a, b = self._n, self._n + m
        self._Y[a:b] = torch.stack([r[1] for r in reqs])
        if self._M is not None:
            self._M[a:b] = torch.stack([r[2] for r in reqs])
        if not self.seeded:
            self._N[a:b] = torch.stack([r[3] for r in reqs])
        self._begin(a, b, [r[0] for r in reqs], [r[3] for r in reqs] if self.seeded else None)

    def _begin(self, a: int, b: int, ids: List[int], keys=None):
        """slots a .. b-1 hold new images (LR planes, mask, draws - or, seeded, their `keys`): ONE rs_sample_begin batch makes their x_T"""
        if self.seeded:   # draw 0 of each key, generated by the kernel that adds it
            noise, kw = None, {"keys": list(keys)}
            self._keys += list(keys)
        else:
            noise, kw = self._N[a:b, 0].contiguous(), {}
        self.engine.sample_begin(self._Y[a:b], noise, self.tables, self.sf, self.scale_factor, prec_encode=self.prec_encode, out=self._X[a:b], **kw)
        self._ids += ids
        self._t += [self.steps - 1] * (b - a)
        self._n = b

    def _admit_rows(self, ids: List[int], draws: List[torch.Tensor], shape, fill):
        """(private: tilepool.py)  Admit len(ids) <= max_batch - active images whose LR planes are ALREADY of the padded shape `shape`
        (hp, wp) and are written in place by `fill(Y_rows [m,3,hp,wp], M_rows [m,1,hp,wp] | None)` - straight into the pool, no staging
        copy; draws[i] [steps+1,Cz,hz,wz] as submit() stacks them - seeded: draws[i] = the image's (seed, stream) key.  Nothing waits in this
        instance's own queue then."""
        m = len(ids)
        assert 0 < m <= self.max_batch - self._n and not self._waiting
        if self._X is None:
            hp, wp = shape
            self._alloc(torch.empty(3, hp, wp, device="meta"), torch.empty(1, hp, wp, device="meta") if self.cond_mask else None,
                        None if self.seeded else draws[0])
        a, b = self._n, self._n + m
        fill(self._Y[a:b], self._M[a:b] if self._M is not None else None)
        if not self.seeded:
            self._N[a:b] = torch.stack(draws)
        self._begin(a, b, list(ids), draws if self.seeded else None)

    def _compact(self, keep: List[int]):
        k = len(keep)
        if k and keep != list(range(k)):
            idx = torch.tensor(keep, device=self.device, dtype=torch.long)
            for P in (self._X, self._Y, self._M, self._N):
                if P is not None:
                    P[:k] = P.index_select(0, idx)
        self._ids = [self._ids[i] for i in keep]
        self._t = [self._t[i] for i in keep]
        self._keys = [self._keys[i] for i in keep] if self.seeded else self._keys
        self._n = k

    def step(self) -> Dict[int, torch.Tensor]:
        """admit -> one step of every active image -> retire; returns {id: image [3, h*sf, w*sf] in [-1,1]} of the images that finished"""
        self._admit()
        ids, img = self._step_batch()
        out: Dict[int, torch.Tensor] = {}
        if ids:
            h, w = self.lr_size
            img = img[:, :, : h * self.sf, : w * self.sf].clamp_(-1.0, 1.0)   # sample_func's crop and clamp
            for j, i in enumerate(ids):
                out[i] = img[j]
        return out

    def _step_batch(self):
        """one step of every active image -> retire: (ids, decoded batch [len(ids),3,hp*sf,wp*sf] of the PADDED shape, not yet clamped) of
        the images that finished, or ([], None)"""
        n = self._n
        if n == 0:
            return [], None
        if self.seeded:   # draw steps - t of each slot's key, generated by the kernel that adds it
            noise, kw = None, {"keys": list(self._keys)}
        else:             # this step's draw of each slot: draw k = steps - t (draw 0 is the prior noise)
            k = torch.tensor([self.steps - t for t in self._t], device=self.device, dtype=torch.long)
            noise, kw = self._N[torch.arange(n, device=self.device), k], {}
        self.engine.sample_step(self._X[:n], self._Y[:n], list(self._t), noise, self.tables, self.sf,
                                mask=self._M[:n] if self._M is not None else None, prec=self.prec_unet, **kw)
        done = [i for i in range(n) if self._t[i] == 0]
        self._t = [t - 1 for t in self._t]
        ids, img = [], None
        if done:
            x0 = self._X[:n].index_select(0, torch.tensor(done, device=self.device, dtype=torch.long))
            hp, wp = self._Y.shape[2], self._Y.shape[3]
            img = self.engine.sample_end(x0, hp, wp, self.sf, self.scale_factor, prec_decode=self.prec_decode, return_aux=self.keep_aux)
            if self.keep_aux:
                img, aux = img
                per = aux["indices"].numel() // len(done)
                for j, i in enumerate(done):
                    self.aux[self._ids[i]] = {"z_final": aux["z_final"][j], "indices": aux["indices"][j * per:(j + 1) * per]}
            ids = [self._ids[i] for i in done]
            self._compact([i for i in range(n) if self._t[i] >= 0])
        return ids, img

    def drain(self) -> Dict[int, torch.Tensor]:
        """step until nothing is waiting or in flight"""
        out: Dict[int, torch.Tensor] = {}
        while self.pending():
            out.update(self.step())
        return out
