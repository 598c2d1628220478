"""Drop-in `ResShiftSampler` (reference: sampler.py:26-308) on top of the HIP engine.

Same constructor and `sample_func` / `inference` signatures as the reference.  Differences that do not
change results: models come from the engine-backed classes (the YAML `target:` strings of the
reference are mapped onto them), every rank can receive the packed weights through ONE RCCL
broadcast instead of re-reading the checkpoint (sharding.py), and image file I/O uses PIL (the
reference uses cv2, which is a host-side detail outside the hot path).

What follows the blend of a whole image - the colour fix, the resize to `out_scale`, their option checks - is `finish.Finish`:
`sample_tiled` calls it on the image it returns, `inference` gets it through `sample_tiled` resp. the `TilePool`.
"""
from __future__ import annotations

import math
import os
import random
from contextlib import nullcontext
from pathlib import Path
from typing import Mapping, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import sharding, tiling
from .autoencoder import VQModelTorch
from .config import ConfigNode, load_config
from .finish import Finish
from .gaussian_diffusion import create_gaussian_diffusion
from .unet import UNetModelSwin

# the reference's only plug-in mechanism is the `target:` string (utils/util_common.py:19-29)
TARGETS = {
    "models.unet.UNetModelSwin": UNetModelSwin,
    "models.script_util.create_gaussian_diffusion": create_gaussian_diffusion,
    "ldm.models.autoencoder.VQModelTorch": VQModelTorch,
    "resshift_amd.unet.UNetModelSwin": UNetModelSwin,
    "resshift_amd.gaussian_diffusion.create_gaussian_diffusion": create_gaussian_diffusion,
    "resshift_amd.autoencoder.VQModelTorch": VQModelTorch,
}


def instantiate_from_config(config: Mapping):
    if "target" not in config:
        raise KeyError("Expected key `target` to instantiate.")
    try:
        cls = TARGETS[config["target"]]
    except KeyError as e:
        raise NotImplementedError(f"target {config['target']} is outside the accelerated hot path") from e
    return cls(**dict(config.get("params", {})))


def reload_model(model: torch.nn.Module, ckpt: Mapping[str, torch.Tensor]) -> None:
    """utils/util_net.py:86-98 semantics: tolerate `module.` / `_orig_mod.` prefixes, require every key."""
    first = next(iter(ckpt.keys()))
    module_flag = first.startswith("module.")
    compile_flag = "_orig_mod" in first
    for key, value in model.state_dict().items():
        tkey = key
        if compile_flag:
            tkey = "_orig_mod." + tkey
        if module_flag:
            tkey = "module." + tkey
        assert tkey in ckpt, f"checkpoint is missing {tkey}"
        value.copy_(ckpt[tkey])


class BaseSampler:
    # precision policies by name: (UNet, encoder, decoder) storage types
    POLICIES = {"parity": ("split", "split", "fp16"), "fp16": ("fp16", "fp16", "fp16"), "fp32": ("fp32", "fp32", "fp32"),
                "split": ("split", "split", "split")}

    def __init__(self, configs, sf=4, use_amp=True, chop_size=128, chop_stride=128, chop_bs=1, padding_offset=16, seed=10000,
                 state_dicts: Optional[Mapping[str, Mapping[str, torch.Tensor]]] = None, blob_cache=None, precision=None, pack="policy",
                 tile_blend="uniform", color_fix="none", out_scale=None):
        """`state_dicts` ({"model": sd, "autoencoder": sd}) replaces checkpoint files, e.g. for synthetic-weight runs.
        `blob_cache`: file that keeps the packed device weights between runs (sharding.build_engine_with_broadcast).
        `precision`: "parity" | "fp16" | "fp32" | "split" (POLICIES).  Default: "parity" when `use_amp` (the reduced-precision path of the
        reference, sampler.py:185 - here the fastest policy that still reproduces the reference's CPU output to >= 60 dB: split-precision
        encoder + UNet, fp16 decoder; the reference's own autocast path, and "fp16" here, flip 2 - 7 % of the VQ codes), "fp32" otherwise.
        `pack`: "policy" - the engine packs, broadcasts and caches only the weight forms that policy needs (a later set_precision to a
        form that was not packed fails loudly); "all" - every form (a process that switches policies).
        `tile_blend`: how overlapping tiles of `sample_tiled` / `inference` (with and without `pool`) are blended: "uniform" - the
        reference's average; "feather" - every tile weighted down towards its own edges across the overlap.  An image of
        one tile is the same under both.
        `color_fix`: "none" | "wavelet" | "adain" - colour correction of every whole image `sample_tiled` / `inference` (with and without
        `pool`) return against its LQ input, on the device (rs_color_fix): "wavelet" keeps the sample's detail and takes the
        low frequencies of the bicubic up-sampled input, "adain" takes the input's per-channel mean and deviation.  Tiles are corrected
        after they are blended, never one by one; `sample_func` is not affected.  Undefined for masked (inpainting) inputs: ValueError.
        `out_scale`: None, or the factor between the LQ input and every whole image `sample_tiled` / `inference` (with and without `pool`)
        return - "x2 from the x4 model", "x3": the image is (ceil(H_lq * out_scale), ceil(W_lq * out_scale)), the model's result resized
        on the device by MATLAB's antialiased bicubic imresize and clamped to [-1, 1] (rs_resize), after the tiles are
        blended and after the colour fix.  None, or a value equal to `sf`, issues exactly the launches issued without it; otherwise
        out_scale / sf must lie in [1/8, 8].  `sample_func` is not affected.  Masked (inpainting) inputs: ValueError."""
        self.configs = configs if isinstance(configs, Mapping) else load_config(configs)
        self.sf = sf
        self.chop_size, self.chop_stride, self.chop_bs = chop_size, chop_stride, chop_bs
        self.seed = seed
        self.use_amp = use_amp
        self.precision = precision if precision is not None else ("parity" if use_amp else "fp32")
        if self.precision not in self.POLICIES:
            raise ValueError(f"unknown precision policy {self.precision!r} (one of {sorted(self.POLICIES)})")
        tiling.check_blend(tile_blend)
        self.tile_blend = tile_blend
        tiling.check_color_fix(color_fix)
        self.color_fix = color_fix
        tiling.check_out_scale(out_scale, sf)
        self.out_scale = out_scale
        if pack not in ("policy", "all"):
            raise ValueError("pack must be 'policy' or 'all'")
        self.pack = pack
        self.padding_offset = padding_offset
        self._state_dicts = state_dicts
        self._blob_cache = blob_cache
        self.setup_dist()
        self.setup_seed()
        self.build_model()

    def setup_seed(self, seed=None):
        seed = self.seed if seed is None else seed
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)

    def setup_dist(self, gpu_id=None):
        """One process per GPU (torchrun); RCCL through torch.distributed backend 'nccl' (sampler.py:66-77)."""
        self.num_gpus, self.rank = sharding.init_distributed()
        self.device = torch.device("cuda", torch.cuda.current_device())

    def write_log(self, log_str):
        if self.rank == 0:
            print(log_str, flush=True)

    def _load_sd(self, which: str, ckpt_path):
        if self._state_dicts is not None and which in self._state_dicts:
            return self._state_dicts[which]
        assert ckpt_path is not None, f"configs.{which}.ckpt_path is required"
        state = torch.load(ckpt_path, map_location="cpu")
        return state["state_dict"] if "state_dict" in state else state

    def build_model(self):
        c = self.configs
        self.write_log(f"Building the diffusion model with length: {c['diffusion']['params']['steps']}...")
        self.base_diffusion = instantiate_from_config(c["diffusion"])
        model = instantiate_from_config(c["model"]).to(self.device)
        autoencoder = instantiate_from_config(c["autoencoder"]).to(self.device) if c.get("autoencoder") is not None else None
        if autoencoder is None:
            raise NotImplementedError("the accelerated path samples in the VQ latent space (all shipped configs)")
        # rank 0 reads + packs the weights once; the packed blob reaches the other ranks by one RCCL broadcast
        eng = sharding.build_engine_with_broadcast(
            model, autoencoder,
            load_fn=lambda: (self._load_sd("model", c["model"].get("ckpt_path")), self._load_sd("autoencoder", c["autoencoder"].get("ckpt_path"))),
            rank=self.rank, world=self.num_gpus, blob_cache=self._blob_cache,
            cache_fingerprint=sharding.checkpoint_fingerprint([c["model"].get("ckpt_path"), c["autoencoder"].get("ckpt_path")]),
            precisions=None if self.pack == "all" else set(self.POLICIES[self.precision]))
        self.base_diffusion.adopt_engine(model, autoencoder, eng)
        self.model = model.eval()
        self.autoencoder = autoencoder.eval()
        self.engine = eng
        self.base_diffusion.set_precision(*self.POLICIES[self.precision])

    def set_precision(self, unet=None, encode=None, decode=None):
        self.base_diffusion.set_precision(unet, encode, decode)


class ResShiftSampler(BaseSampler):
    def sample_func(self, y0, noise_repeat=False, mask=False, noise=None, step_noises=None, seeds=None):
        """y0: [n,c,h,w] in [-1,1]; returns [n,c,h*sf,w*sf] in [-1,1] (sampler.py:119-165).  `seeds`: one int or (seed, stream) pair per
        image - per-request noise generated inside the engine (p_sample_loop's seeds=) instead of torch.randn / tensors."""
        if noise_repeat:
            self.setup_seed()
        if mask is False:
            mask = None
        offset = self.padding_offset
        ori_h, ori_w = y0.shape[2:]
        flag_pad = not (ori_h % offset == 0 and ori_w % offset == 0)
        if flag_pad:
            pad_h = (math.ceil(ori_h / offset)) * offset - ori_h
            pad_w = (math.ceil(ori_w / offset)) * offset - ori_w
            y0 = sharding.reflect_pad(y0, pad_h, pad_w)
            if mask is not None:
                # (deviation: the reference pads y0 only, sampler.py:130-138, and then fails in the UNet's channel concat when an
                # inpainting input needs padding; padding the mask alike keeps such inputs usable and changes nothing otherwise)
                mask = sharding.reflect_pad(mask, pad_h, pad_w)
        cond_lq = self.configs["model"]["params"].get("cond_lq", True)
        if cond_lq and mask is not None:
            model_kwargs = {"lq": y0, "mask": mask}
        elif cond_lq:
            model_kwargs = {"lq": y0}
        else:
            model_kwargs = None
        results = self.base_diffusion.p_sample_loop(y=y0, model=self.model, first_stage_model=self.autoencoder, noise=noise,
                                                    noise_repeat=noise_repeat, clip_denoised=(self.autoencoder is None),
                                                    denoised_fn=None, model_kwargs=model_kwargs, progress=False,
                                                    step_noises=step_noises, **({"seeds": seeds} if seeds is not None else {}))
        if flag_pad:
            results = results[:, :, : ori_h * self.sf, : ori_w * self.sf]
        return results.clamp_(-1.0, 1.0)

    def image_seed(self, index: int) -> int:
        """The seed `inference(seeded=True)` gives the image at position `index` of the sorted listing of the WHOLE input (not of a rank's
        share): continuous.request_seed(self.seed, index) = (self.seed * 2^32 + index) mod 2^64."""
        from .continuous import request_seed

        return request_seed(self.seed, index)

    def sample_tiled(self, im_lq, mask=None, noise_repeat=False, tile_noises=None, seed=None):
        """sampler.py:176-216 (`_process_per_image`): inputs larger than `chop_size` are cut into overlapping
        `chop_size` tiles (stride `chop_stride`, `chop_bs` tiles per sampler call), sampled independently and
        overlap-averaged on the GPU; smaller inputs go straight to `sample_func`.  Returns [-1,1] like sample_func.
        `tile_noises[k] = (noise, step_noises)` injects the draws of the k-th sampler call (parity runs).
        `seed` (an int, or one per image of the batch): tile j of an image (index in tiling.extract_starts order) draws its noise from
        key (seed, stream = j) - what tilepool.TilePool(seeded=True) gives the same image; an untiled image is its tile 0."""
        from .tiling import TileSplitter

        finish = Finish.of(self)   # (per call: the options may change between calls)
        if mask is not None:
            finish.reject_mask("sample_tiled")
        engine = getattr(self, "engine", None)   # (only a fix or a resize reaches it)
        B0 = im_lq.shape[0]
        if seed is not None:
            if tile_noises is not None or noise_repeat:
                raise ValueError("seed= names every draw: it excludes tile_noises and noise_repeat")
            seeds = [int(v) for v in seed] if isinstance(seed, (list, tuple)) else [int(seed)] * B0
            if len(seeds) != B0:
                raise ValueError(f"seed: {B0} images but {len(seeds)} seeds")
        if not (im_lq.shape[2] > self.chop_size or im_lq.shape[3] > self.chop_size):
            if seed is not None:
                sr = self.sample_func(im_lq, mask=mask, seeds=[(sd, 0) for sd in seeds])
            else:
                nz = tile_noises[0] if tile_noises else (None, None)
                sr = self.sample_func(im_lq, noise_repeat=noise_repeat, mask=mask, noise=nz[0], step_noises=nz[1])
            return finish(engine, sr, im_lq)
        x = torch.cat([im_lq, mask], dim=1) if mask is not None else im_lq
        splitter = TileSplitter(x, self.chop_size, stride=self.chop_stride, sf=self.sf, extra_bs=self.chop_bs,
                                **({"blend": finish.blend} if finish.blend != "uniform" else {}))   # ("uniform": the call as it always was)
        for k, (pch, index_infos) in enumerate(splitter):
            if mask is not None:
                pch, mask_pch = pch[:, :-1].contiguous(), pch[:, -1:].contiguous()
            else:
                mask_pch = None
            if seed is not None:   # rows of this call: tile k * chop_bs + kk, image b at row kk * B0 + b (TileSplitter.__next__)
                keys = [(seeds[b], k * self.chop_bs + kk) for kk in range(len(index_infos)) for b in range(B0)]
                out = self.sample_func(pch, mask=mask_pch, seeds=keys)
            else:
                nz = tile_noises[k] if tile_noises else (None, None)
                out = self.sample_func(pch, noise_repeat=noise_repeat, mask=mask_pch, noise=nz[0], step_noises=nz[1])
            splitter.update(out, index_infos)
        return finish(engine, splitter.gather(), im_lq)

    # ------------------------------------------------------------------ file-level demo driver
    @staticmethod
    def _read_image_u8(path, gray=False) -> torch.Tensor:
        """uint8 HWC tensor (RGB, or one channel for masks); decoding is host work, everything after it runs on the GPU."""
        from PIL import Image

        im = np.asarray(Image.open(path).convert("L" if gray else "RGB"), dtype=np.uint8)
        return torch.from_numpy(im.reshape(im.shape[0], im.shape[1], -1).copy())

    POOL_LOOKAHEAD = 128   # inference(pool=True) reads files ahead until this many tiles wait for a slot

    # ------------------------------------------------------------------ scores against ground truth
    @staticmethod
    def _gt_file(gt_path, p, single) -> Path:
        """the ground truth of the input file `p`: looked up by file name in the directory `gt_path`; for a single input file `gt_path` is
        the file itself (the rule of `mask_path`)"""
        g = Path(gt_path) if single else Path(gt_path) / Path(p).name
        if not g.is_file():
            raise FileNotFoundError(f"no ground truth for {Path(p).name}: {g} is not a file")
        return g

    def _score(self, out_u8, files, gt_path, single, border, ycbcr) -> dict:
        """{stem: (psnr, ssim)} of the uint8 device batch out_u8 [n,H,W,C] - the very pixels that become the PNGs of `files` - against
        their ground-truth files: read on the host, scored on the device (Engine.metrics).  A gray output is its own luma."""
        gray = out_u8.shape[3] == 1
        gts = []
        for p, im in zip(files, out_u8):
            g = self._read_image_u8(self._gt_file(gt_path, p, single), gray=gray)
            if tuple(g.shape) != tuple(im.shape):
                raise ValueError(f"the ground truth of {Path(p).name} is {g.shape[0]} x {g.shape[1]}, the output is {im.shape[0]} x {im.shape[1]}")
            gts.append(g)
        m = self.engine.metrics(out_u8, torch.stack(gts).to(self.device), border=border, ycbcr=bool(ycbcr) and not gray)
        psnr, ssim = m["psnr"].cpu().tolist(), m["ssim"].cpu().tolist()
        return {Path(p).stem: (float(a), float(b)) for p, a, b in zip(files, psnr, ssim)}

    @staticmethod
    def _write_metrics(out_path, rows) -> tuple:
        """out_path/metrics.csv: name,psnr,ssim - one row per image sorted by name, then the row `mean`; returns the two means"""
        names = sorted(rows)
        mean = tuple(float(np.mean([rows[k][i] for k in names])) if names else float("nan") for i in (0, 1))
        with open(Path(out_path) / "metrics.csv", "w") as fh:
            fh.write("name,psnr,ssim\n")
            for k in names:
                fh.write(f"{k},{rows[k][0]!r},{rows[k][1]!r}\n")
            fh.write(f"mean,{mean[0]!r},{mean[1]!r}\n")
        return mean

    def _finish_metrics(self, out_path, rows) -> dict:
        """the rows of every rank combined (all_gather_object); rank 0 writes metrics.csv and logs the means; every rank returns all rows"""
        if self.num_gpus > 1 and dist.is_available() and dist.is_initialized():
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, rows)
            rows = {k: v for part in parts for k, v in part.items()}
        if self.rank == 0:
            mean = self._write_metrics(out_path, rows)
            self.write_log(f"{len(rows)} images against ground truth: mean PSNR {mean[0]:.4f} dB, mean SSIM {mean[1]:.6f} ({Path(out_path) / 'metrics.csv'})")
        return rows

    def inference(self, in_path, out_path, mask_path=None, mask_back=True, bs=1, noise_repeat=False, pool=False, seeded=False, gt_path=None,
                  metric_border=0, metric_ycbcr=True, out_ext="png", jpeg_quality=95):
        """sampler.py:167-308: batches of `bs` images are sharded over the ranks exactly like sampler.py:273-277; every
        rank writes its own PNGs.  uint8 -> [-1,1] (datapipe/datasets.py:59-63), the inpainting blend (sampler.py:218-222)
        and the final clamp / round to uint8 (utils/util_image.py:245-269) run on the device (rs_u8_to_input /
        rs_output_to_u8): only uint8 pixels cross PCIe.  Inputs larger than `chop_size` take the tiled path.
        `pool=True`: the files of this rank's share (same sharding) are read one by one - their sizes may differ - and submitted to ONE
        `tilepool.TilePool`, whose batches hold tiles of several images; each PNG is written when its image completes.  Files are
        submitted ahead while fewer than POOL_LOOKAHEAD tiles wait, then the pool steps.
        `seeded=True` (with and without `pool`): the image at position i of the sorted listing of the whole input gets the seed
        `image_seed(i)`, its tile j the stream j - the noise of a file does not depend on the number of ranks, on `bs` or
        on `pool`, so neither do the PNGs beyond the engine's own batch-size sensitivity.  Excludes `noise_repeat`.
        The sampler's `color_fix` and `out_scale` reach every image through `sample_tiled` resp. the `TilePool`; they exclude `mask_path`.
        `gt_path` (None: nothing changes, None is returned): every image is scored against its ground truth - the file of the same name in
        that directory, or `gt_path` itself for a single input file - on the device, from the very uint8 tensor that becomes its PNG (after
        the inpainting blend, the colour fix and `out_scale`): PSNR and SSIM as the reference's calculate_psnr / calculate_ssim compute
        them (Engine.metrics), `metric_border` pixels cropped, on MATLAB's Y channel when `metric_ycbcr`.  Returns
        {stem: (psnr, ssim)} for the whole input on every rank; rank 0 writes out_path/metrics.csv.  A missing ground-truth file raises
        FileNotFoundError before anything is sampled, one of another size than the output ValueError.
        `out_ext`: "png" (the default: the PNGs above, not a launch or a byte changed) or "jpg": every image is written as
        out_path/{stem}.jpg, a baseline JPEG at `jpeg_quality` (an integer 1 .. 100) coded on the device from the same uint8 tensor
        (Engine.jpeg_encode, DESIGN.md 7j: the bytes of PIL's save(quality=jpeg_quality, subsampling=2)), on the batch, the tiled and the
        `pool` route alike - only compressed bytes cross PCIe.  With `gt_path` the scores remain those of that uint8 tensor, the image
        BEFORE the JPEG coding; the file on disk is its JPEG.  A one-channel output has no JPEG here: ValueError before anything is
        sampled or written, like any other `out_ext` and a `jpeg_quality` outside 1 .. 100."""
        if seeded and noise_repeat:
            raise ValueError("seeded=True names every draw by (seed, stream): it excludes noise_repeat")
        if out_ext not in ("png", "jpg"):
            raise ValueError(f"out_ext must be 'png' or 'jpg', not {out_ext!r}")
        if out_ext == "jpg":
            if isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, int) or not 1 <= jpeg_quality <= 100:
                raise ValueError(f"jpeg_quality must be an integer in 1 .. 100, not {jpeg_quality!r}")
            out_ch = int(self.configs["autoencoder"]["params"]["ddconfig"]["out_ch"])
            if out_ch != 3:
                raise ValueError(f"out_ext='jpg' needs a three-channel (RGB) output; this model's has {out_ch}")
        finish = Finish.of(self)   # (the options are checked before anything is touched; sample_tiled and the TilePool build their own)
        if mask_path is not None:
            finish.reject_mask("inference")
        in_path, out_path = Path(in_path), Path(out_path)
        if self.rank == 0:
            out_path.mkdir(parents=True, exist_ok=True)
        sharding.barrier()
        single = not in_path.is_dir()
        if single:
            files = [in_path]
        else:
            # utils/util_common.py:68-87 with recursive=True (sampler.py:246,258): one recursive glob per extension, in the
            # reference's extension order, each sorted; the inpainting loader adds 'PNG' (sampler.py:259)
            exts = ["png", "jpg", "jpeg", "JPEG", "bmp"] + (["PNG"] if mask_path is not None else [])
            files = [p for e in exts for p in sorted(in_path.glob(f"**/*.{e}"))]
        rows = None
        if gt_path is not None:
            if isinstance(metric_border, bool) or not isinstance(metric_border, int) or metric_border < 0:
                raise ValueError(f"metric_border must be a non-negative integer, not {metric_border!r}")
            for p in files:
                self._gt_file(gt_path, p, single)
            rows = {}
        score = (lambda u8, fs: rows.update(self._score(u8, fs, gt_path, single, metric_border, metric_ycbcr))) if rows is not None else None
        load = lambda fs: self._load(fs, mask_path, single)
        if out_ext == "png":
            write = lambda sr, lq, mask, fs: self._write_pngs(sr, lq, mask, mask_back, fs, out_path, score)
        else:
            write = lambda sr, lq, mask, fs: self._write_jpgs(sr, lq, mask, mask_back, fs, out_path, jpeg_quality, score)
        if pool:
            self._inference_pool(self._shares(files, bs), load, write, noise_repeat, seeded)
        else:
            for first, mine in self._shares(files, bs):
                lq, mask = load(mine)
                if seeded:
                    sr = self.sample_tiled(lq, mask=mask, seed=[self.image_seed(first + j) for j in range(len(mine))])
                else:
                    sr = self.sample_tiled(lq, mask=mask, noise_repeat=noise_repeat)
                write(sr, lq, mask, mine)
        sharding.barrier()
        if rows is not None:
            rows = self._finish_metrics(out_path, rows)
        self.write_log(f"Processing done, enjoy the results in {out_path}")
        return rows

    def make_lq(self, gt_path, lq_path, opts=None, seed=None) -> dict:
        """A folder of ground-truth images -> a folder of LQ PNGs plus plans.json, by the reference's Real-ESRGAN degradation on the device
        (degrade.make_testset) with this sampler's `sf`, seed and device; the listing is sharded over the ranks like
        `inference`'s, rank 0 writes plans.json.  Then `inference(lq_path, out, gt_path=gt_path)` closes the loop.  Returns {stem: plan}
        for the whole input on every rank.  `opts=degrade.FACE_TESTING` (a FaceOptions): the face recipe instead (degrade.make_face_testset,
        DESIGN.md 7i), whose LQ images keep the ground truth's size."""
        from . import degrade

        files = degrade.list_images(gt_path)
        mine = [first + j for first, part in self._shares(files, self.num_gpus) for j in range(len(part))]
        common = dict(seed=self.seed if seed is None else seed, device=getattr(self, "engine", None) or self.device, positions=mine)
        if isinstance(opts, degrade.FaceOptions):   # the face recipe: LQ images of the ground truth's size
            plans = degrade.make_face_testset(gt_path, lq_path, opts=opts, **common)
        else:
            plans = degrade.make_testset(gt_path, lq_path, sf=self.sf, opts=degrade.REALESRGAN_TESTING if opts is None else opts, **common)
        if self.num_gpus > 1 and dist.is_available() and dist.is_initialized():
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, plans)
            plans = {k: v for part in parts for k, v in part.items()}
        if self.rank == 0:
            degrade.write_plans(lq_path, plans)
        sharding.barrier()
        return plans

    def _shares(self, files, bs):
        """(position of mine[0] in the whole listing, mine) for every batch of `bs` files that gives this rank a share `mine`"""
        micro = math.ceil(bs / self.num_gpus)   # sampler.py:274-277: the slice width comes from bs, also on the last, partial batch
        for b0 in range(0, len(files), bs):
            mine = files[b0:b0 + bs][self.rank * micro:(self.rank + 1) * micro]
            if mine:
                yield b0 + self.rank * micro, mine

    def _load(self, files, mask_path, single):
        """(lq [n,3,H,W], mask [n,1,H,W] | None) of `files` in [-1,1] on the device.  A directory input looks the mask up by file name
        (datapipe/datasets.py:470); a single input file takes mask_path as the mask file itself (sampler.py:296-297)."""
        lq = self.engine.u8_to_input(torch.stack([self._read_image_u8(p) for p in files]).to(self.device))
        if mask_path is None:
            return lq, None
        mpaths = [Path(mask_path)] if single else [Path(mask_path) / p.name for p in files]
        return lq, self.engine.u8_to_input(torch.stack([self._read_image_u8(m, gray=True) for m in mpaths]).to(self.device))

    def _output_u8(self, sr, lq, mask, mask_back, files, score=None):
        """the finished batch sr [n,C,H,W] of `files` -> uint8 [n,H,W,C] on the device: the inpainting blend and the rounding there,
        `score(u8, files)` on the very tensor that is then written"""
        blend = mask is not None and mask_back
        out_u8 = self.engine.output_to_u8(sr, lq=lq if blend else None, mask=mask if blend else None)
        if score is not None:
            score(out_u8, files)
        return out_u8

    def _write_pngs(self, sr, lq, mask, mask_back, files, out_path, score=None):
        """the finished batch of `files` -> their PNGs: the uint8 pixels cross PCIe, Pillow encodes on the host"""
        from PIL import Image

        for p, im in zip(files, self._output_u8(sr, lq, mask, mask_back, files, score).cpu().numpy()):
            Image.fromarray(im if im.shape[2] != 1 else im[:, :, 0]).save(out_path / f"{p.stem}.png")

    def _write_jpgs(self, sr, lq, mask, mask_back, files, out_path, quality, score=None):
        """`_write_pngs` for out_ext="jpg": the same uint8 device tensor, coded to JPEG files on the device - only their bytes cross PCIe"""
        for p, data in zip(files, self.engine.jpeg_encode(self._output_u8(sr, lq, mask, mask_back, files, score), quality)):
            (out_path / f"{p.stem}.jpg").write_bytes(data)

    def _inference_pool(self, shares, load, write, noise_repeat, seeded):
        """the files of `shares`, one by one, through ONE TilePool: submitted ahead while fewer than POOL_LOOKAHEAD tiles wait; an image
        is written when it completes"""
        from .tilepool import TilePool

        if noise_repeat:
            raise NotImplementedError("noise_repeat shares one draw across a batch; the tile pool has no fixed batch")
        tp = TilePool(self, seeded=seeded)
        kept = {}   # image id -> (file, lq, mask) until its PNG is written

        def step():
            for rid, sr in tp.step().items():
                p, lq, mask = kept.pop(rid)
                write(sr.unsqueeze(0), lq, mask, [p])

        for first, mine in shares:
            for j, p in enumerate(mine):
                lq, mask = load([p])
                kept[tp.submit(lq, mask=mask, seed=self.image_seed(first + j) if seeded else None)] = (p, lq, mask)
                while tp.waiting_tiles() >= self.POOL_LOOKAHEAD:
                    step()
        while tp.pending():
            step()
