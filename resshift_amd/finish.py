"""What follows the blend of a whole image, for every route an image can take (`ResShiftSampler.sample_tiled`, `inference` with and
without the pool, `tilepool.TilePool`): the colour fix at the model's scale, then the resize to `out_scale` (7f) - whole
images only, never a tile.  The sampler's `tile_blend` (7d) travels along, since the same three options are read, defaulted and checked
together.  The next whole-image feature hooks in here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

from . import tiling


@dataclass(frozen=True)
class Finish:
    sf: Optional[int]
    blend: str
    color_fix: str
    out_scale: object   # as the sampler holds it
    resize_to: object   # `out_scale` where it asks for another size than the model's, else None

    @classmethod
    def of(cls, sampler, sf=None) -> "Finish":
        """The options of `sampler`, validated; a sampler that lacks an attribute gets the value that issues exactly the calls issued
        before the option existed.  `sf`: the model's scale where the caller holds it itself (TilePool: the diffusion's); only an
        `out_scale` needs one."""
        sf = getattr(sampler, "sf", None) if sf is None else sf
        blend = getattr(sampler, "tile_blend", "uniform")
        fix = getattr(sampler, "color_fix", "none")
        out_scale = getattr(sampler, "out_scale", None)
        tiling.check_blend(blend)
        tiling.check_color_fix(fix)
        tiling.check_out_scale(out_scale, sf)
        return cls(sf, blend, fix, out_scale, out_scale if tiling.resizes(out_scale, sf) else None)

    def reject_mask(self, context: str) -> None:
        """a masked (inpainting) input excludes both steps; `context`: "sample_tiled" | "inference" | "TilePool" """
        where, why_fix, why_scale = {
            "sample_tiled": ("a masked input", " (the LQ image has a hole): use color_fix='none'", " (lq and mask stay at the model's size): use out_scale=None"),
            "inference": ("masked (inpainting) inputs", ": use color_fix='none'", ": use out_scale=None"),
            "TilePool": ("a model conditioned on a mask", " (the LQ image has a hole)", " (lq and mask stay at the model's size)"),
        }[context]
        if self.color_fix != "none":
            raise ValueError(f"color_fix={self.color_fix!r} is undefined for {where}{why_fix}")
        if self.resize_to is not None:
            raise ValueError(f"out_scale={self.resize_to!r} is undefined for {where}{why_scale}")

    def __call__(self, engine, sr, lq):
        """sr [B,C,H*sf,W*sf], lq [B,C,H,W] -> the finished images; under ("none", no resize) no engine call, and `sr` itself"""
        if self.color_fix != "none":
            sr = engine.color_fix(sr, lq, self.color_fix)
        if self.resize_to is not None:
            sr = engine.resize(sr, size=tiling.out_size(lq.shape[2], lq.shape[3], self.resize_to), clamp=True)
        return sr
