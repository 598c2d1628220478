"""Tile pool: whole LR images of any size, arriving at any time, through the continuous-batching sampler.

`ResShiftSampler.sample_tiled` cuts ONE image into overlapping tiles and samples them `chop_bs` at a time, so an image with few tiles -
or a folder of images of different sizes - never fills a batch.  Tiles are independent units, every tile of an image has the same LR
shape and nothing in the network mixes batch entries, so `TilePool` pools the tiles of ALL pending images:

  * `submit(lq)` cuts the image into the tiles `tiling.TileSplitter` would cut (`tiling.extract_starts`, the sampler's `chop_size` /
    `chop_stride`, the same clamped windows; an image at or below `chop_size` in both directions is one tile, as `sample_tiled` sends it
    straight to `sample_func`) and draws - or takes - every tile's noises;
  * a tile's **size class** is its padded LR shape (`ceil(th / padding_offset) * padding_offset`, likewise `tw`: what `sample_func` pads
    it to).  Each class has its own dense pool, a `ContinuousSampler`; tiles of different images - and of images of different sizes -
    share a batch whenever their class is the same.  Tiles wait in FIFO order: image submit order, then tile index order;
  * `step()` advances ONE class: the class that holds the oldest unfinished tile (lowest (image, tile index) among the tiles waiting or
    in flight).  It admits waiting tiles of that class into the free slots of its pool (ONE `rs_tile_gather` launch crops and
    reflect-pads them, mask included, straight into the pool's rows; one `rs_sample_begin`), runs one `rs_sample_step` over the pool,
    decodes the tiles that finished (one `rs_sample_end`), clamps them as `sample_func` does and adds them into their images' canvases
    with ONE `rs_tile_scatter` launch - the bits of `rs_tile_accumulate` called tile by tile in index order, whichever images the
    tiles belong to.  An image whose last tile has retired is divided by its counts (`rs_tile_finalize`; a one-tile image alike: a sum
    of one divided by one) and returned.

Per-tile arithmetic is the engine's per-image arithmetic at that batch size: an image whose tiles make up one batch comes out bit for
bit as `sample_tiled` with `chop_bs` = that batch.  The restrictions of `ContinuousSampler` carry over: no `noise_repeat` (it is defined
by a fixed batch; unsupported with tensors and with seeds alike), one UNet
precision for every step, latent-space models.  Out of scope: images of different sizes inside one UNet batch, one pool across ranks.

The blend is the sampler's `tile_blend`: "uniform" (default, the reference's average, the launches above) or "feather" (DESIGN.md 7d):
tiles retire through ONE `rs_tile_scatter_weighted` launch - the bits of `rs_tile_accumulate_weighted` tile by tile, which is what
`sample_tiled` issues under the same mode - and the count plane holds the weight sum that `rs_tile_finalize` divides by.

The sampler's `color_fix` ("none" by default) is applied to each completed image after `rs_tile_finalize`, against the
image's own LQ planes (`rs_color_fix`): tiles are never corrected one by one.  The sampler's `out_scale` (None by default)
follows it: each completed image is resized to (ceil(H * out_scale), ceil(W * out_scale)) and clamped (`rs_resize`).  Both are
`finish.Finish`, the one stage `sample_tiled` runs too; `step()` calls it where an image completes.

`seeded=True`: `submit(image, seed=...)` names the image; tile j (index in `tiling.extract_starts` order, the order of
`tile_windows`) draws its noise from key (seed, stream = j) inside the engine's kernels.  No draws are made or stored, and an image's
tiles get the same noise whatever else is pending, whichever pool or rank serves them, and in `ResShiftSampler.sample_tiled(seed=)`.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .continuous import ContinuousSampler, check_sampler, request_seed
from .finish import Finish
from .tiling import extract_starts, feather_ramp

HEADLINE_PIXELS = 32 * 64 * 64   # LR pixels of the benchmark's batch (32 images of 64 x 64): what `max_batch=None` fills a class up to


def tile_windows(H: int, W: int, chop_size: int, chop_stride: int) -> List[Tuple[int, int, int, int]]:
    """(h0, w0, th, tw) of every tile of an H x W image, in TileSplitter's order (rows of tiles, then columns); th = min(chop_size, H)."""
    th, tw = min(chop_size, H), min(chop_size, W)
    return [(h0, w0, th, tw) for h0 in extract_starts(H, chop_size, chop_stride) for w0 in extract_starts(W, chop_size, chop_stride)]


def class_key(th: int, tw: int, padding_offset: int) -> Tuple[int, int]:
    """padded LR shape of a th x tw tile (sampler.py:130-138)"""
    return (math.ceil(th / padding_offset) * padding_offset, math.ceil(tw / padding_offset) * padding_offset)


class _Image:
    __slots__ = ("id", "src", "H", "W", "left", "acc", "count")

    def __init__(self, id_, src, n_tiles):
        self.id, self.src, self.H, self.W, self.left = id_, src, int(src.shape[1]), int(src.shape[2]), n_tiles
        self.acc = self.count = None   # canvases: allocated when the first tile retires


class _Class:
    __slots__ = ("cs", "waiting")

    def __init__(self, cs):
        self.cs, self.waiting = cs, deque()   # waiting: tile sequence numbers, ascending


class TilePool:
    def __init__(self, sampler, max_batch: Optional[int] = None, keep_log: bool = False, seeded: bool = False):
        """`max_batch`: most tiles of one class in flight.  None: clamp(32 * 64*64 // (Hp * Wp), 1, 32) per class - the LR pixel count of
        the benchmark's batch; an explicit value holds for every class, up to RS_MAX_ROWS.  `keep_log`: record in `self.batches`, per
        engine step, the (image id, tile index) of every row the step held.  `seeded`: images carry a seed instead of noise tensors
        (module docstring)."""
        check_sampler(sampler, max_batch, who="TilePool")
        self.sampler, self.max_batch = sampler, (int(max_batch) if max_batch is not None else None)
        d = sampler.base_diffusion
        self.chop_size, self.chop_stride = int(sampler.chop_size), int(sampler.chop_stride)
        if self.chop_stride > self.chop_size:
            raise ValueError("chop_stride must not exceed chop_size (tiles would leave gaps)")
        self.offset, self.sf, self.steps = int(sampler.padding_offset), int(d.sf), int(d.num_timesteps)
        self.cond_mask = bool(sampler.configs["model"]["params"].get("cond_mask", False))
        self.device = getattr(sampler, "device", None) or torch.device("cuda", torch.cuda.current_device())
        self.engine = sampler.engine
        self._classes: Dict[Tuple[int, int], _Class] = {}
        self._images: Dict[int, _Image] = {}
        self._tiles: Dict[int, tuple] = {}   # tile sequence number -> (image, (h0, w0, th, tw), class key, draws [steps+1,Cz,hz,wz])
        self._next_image = self._next_tile = 0
        self.keep_log, self.batches = bool(keep_log), []
        self.seeded = bool(seeded)
        # the blend ("feather" retires tiles through rs_tile_scatter_weighted), and what follows it on each completed image - the colour
        # fix, then the output scale - are the sampler's (finish.py)
        self.finish = Finish.of(sampler, sf=self.sf)
        if self.cond_mask:
            self.finish.reject_mask("TilePool")
        self.blend, self.color_fix, self.out_scale = self.finish.blend, self.finish.color_fix, self.finish.out_scale
        self.ramp = feather_ramp(self.chop_size, self.chop_stride, self.sf) if self.blend == "feather" else None
        self._tile_index: Dict[int, int] = {}

    # ------------------------------------------------------------------ requests
    def class_max_batch(self, key: Tuple[int, int]) -> int:
        if self.max_batch is not None:
            return self.max_batch
        return max(1, min(32, HEADLINE_PIXELS // (key[0] * key[1])))

    def submit(self, lq, mask=None, tile_noises=None, seed=None) -> int:
        """Queue one LR image lq [3,H,W] (or [1,3,H,W]) in [-1,1], with its mask [1,H,W] where the model takes one; returns its id.
        `tile_noises[k] = (noise [Cz,hz,wz], step_noises: steps tensors alike, in loop order)` injects tile k's draws (a leading batch
        axis of 1 is accepted); otherwise they are drawn now, tile by tile in index order - one torch.randn of [steps+1,Cz,hz,wz] per tile,
        row 0 the prior noise, row k the draw of the k-th loop iteration - so a run under torch.manual_seed is reproducible.
        Seeded mode: `seed` (default request_seed(sampler.seed, image id)) names the image, tile j uses stream j; tile_noises is rejected."""
        if self.seeded and tile_noises is not None:
            raise ValueError("a seeded TilePool generates its noise from seeds: tile_noises tensors are not accepted")
        if not self.seeded and seed is not None:
            raise ValueError("seed= needs TilePool(..., seeded=True)")
        if lq.dim() == 4:
            if lq.shape[0] != 1:
                raise ValueError("TilePool.submit takes ONE image (sizes may differ between images): submit them one by one")
            lq = lq[0]
            mask = mask[0] if mask is not None and mask.dim() == 4 else mask
        if lq.dim() != 3 or lq.shape[0] != 3:
            raise ValueError(f"lq must be [3,H,W], got {tuple(lq.shape)}")
        if self.cond_mask and mask is None:
            raise ValueError("this model is conditioned on a mask (cond_mask): submit(lq, mask=...)")
        H, W = int(lq.shape[1]), int(lq.shape[2])
        lq = lq.to(self.device, torch.float32)
        if self.cond_mask:   # the mask travels as fourth plane, as sample_tiled concatenates it
            if mask.dim() == 2:
                mask = mask.unsqueeze(0)
            if tuple(mask.shape) != (1, H, W):
                raise ValueError(f"mask must be [1,{H},{W}], got {tuple(mask.shape)}")
            src = torch.cat([lq, mask.to(self.device, torch.float32)], 0)
        else:
            src = lq.contiguous()
        wins = tile_windows(H, W, self.chop_size, self.chop_stride)
        key = class_key(wins[0][2], wins[0][3], self.offset)
        if key[0] - wins[0][2] >= wins[0][2] or key[1] - wins[0][3] >= wins[0][3]:
            raise ValueError(f"a {wins[0][2]}x{wins[0][3]} tile cannot be reflect-padded to {key[0]}x{key[1]}: the padding must be smaller "
                             "than the padded side (as torch.nn.functional.pad requires)")
        if tile_noises is not None and len(tile_noises) != len(wins):
            raise ValueError(f"tile_noises: this image has {len(wins)} tiles, got draws for {len(tile_noises)}")
        zs = tuple(self.engine.latent_shape(1, key[0], key[1], self.sf))[1:]
        draws = []
        if self.seeded:
            sd = int(seed if seed is not None else request_seed(getattr(self.sampler, "seed", 0), self._next_image)) % 2 ** 64
            draws = [(sd, j) for j in range(len(wins))]
        for k in range(len(wins) if not self.seeded else 0):
            if tile_noises is None:
                draws.append(torch.randn((self.steps + 1,) + zs, device=self.device, dtype=torch.float32))
            else:
                noise, step_noises = tile_noises[k]
                if len(step_noises) != self.steps:
                    raise ValueError(f"tile_noises[{k}]: {self.steps} step draws expected, got {len(step_noises)}")
                draws.append(torch.stack([t.to(self.device, torch.float32).reshape(zs) for t in [noise, *step_noises]]))
        im = _Image(self._next_image, src, len(wins))
        self._next_image += 1
        if key not in self._classes:
            self._classes[key] = _Class(ContinuousSampler(self.sampler, max_batch=self.class_max_batch(key), seeded=self.seeded))
        for k, win in enumerate(wins):
            self._tiles[self._next_tile] = (im, win, key, draws[k])
            self._tile_index[self._next_tile] = k
            self._classes[key].waiting.append(self._next_tile)
            self._next_tile += 1
        self._images[im.id] = im
        return im.id

    def pending(self) -> int:
        """images submitted and not yet returned"""
        return len(self._images)

    def waiting_tiles(self) -> int:
        """tiles not yet admitted to a pool"""
        return sum(len(c.waiting) for c in self._classes.values())

    # ------------------------------------------------------------------ scheduling
    def _oldest_class(self) -> Optional[Tuple[int, int]]:
        best, best_key = None, None
        for key, c in self._classes.items():
            cand = ([c.waiting[0]] if c.waiting else []) + ([min(c.cs._ids)] if c.cs._ids else [])
            if cand and (best is None or min(cand) < best):
                best, best_key = min(cand), key
        return best_key

    def _admit(self, key, c: _Class):
        m = min(len(c.waiting), c.cs.max_batch - c.cs.active)
        if m <= 0:
            return
        seqs = [c.waiting.popleft() for _ in range(m)]
        rows = [(self._tiles[s][0].src, *self._tiles[s][1]) for s in seqs]
        c.cs._admit_rows(seqs, [self._tiles[s][3] for s in seqs], key, lambda Y, M: _lib.tile_gather(rows, Y, M))
        for s in seqs:   # the pool's rows hold the draws now
            self._tiles[s] = self._tiles[s][:3] + (None,)

    def step(self) -> Dict[int, torch.Tensor]:
        """One engine step of the class that holds the oldest unfinished tile: admit -> step -> retire -> overlap-add.  Returns
        {id: image [3, H*sf, W*sf] in [-1,1]} of the images whose last tile retired in this step."""
        key = self._oldest_class()
        if key is None:
            return {}
        c = self._classes[key]
        self._admit(key, c)
        if self.keep_log:
            self.batches.append([(self._tiles[s][0].id, self._tile_index[s]) for s in c.cs._ids])
        seqs, batch = c.cs._step_batch()
        out: Dict[int, torch.Tensor] = {}
        if not seqs:
            return out
        batch.clamp_(-1.0, 1.0)   # sample_func's clamp (its crop is the scatter's window)
        rows, done = [], []
        for s in seqs:
            im, (h0, w0, th, tw), _, _ = self._tiles.pop(s)
            self._tile_index.pop(s)
            if im.acc is None:
                im.acc = torch.zeros(batch.shape[1], im.H * self.sf, im.W * self.sf, device=batch.device, dtype=torch.float32)
                im.count = torch.zeros(im.H * self.sf, im.W * self.sf, device=batch.device, dtype=torch.float32)
            rows.append((im.acc, im.count, im.H, im.W, h0, w0, th, tw))
            im.left -= 1
            if im.left == 0:
                done.append(im)
        if self.ramp is None:
            _lib.tile_scatter(rows, batch, self.sf)
        else:
            _lib.tile_scatter(rows, batch, self.sf, ramp=self.ramp)
        for im in done:
            res = _lib.tile_finalize(im.acc, im.count)
            # the whole image against its own LQ planes (no mask plane), never a tile
            res = self.finish(self.engine, res.unsqueeze(0), im.src[:3].unsqueeze(0))[0]
            out[im.id] = res
            del self._images[im.id]
        return out

    def drain(self) -> Dict[int, torch.Tensor]:
        """step until every submitted image has been returned"""
        out: Dict[int, torch.Tensor] = {}
        while self.pending():
            out.update(self.step())
        return out
