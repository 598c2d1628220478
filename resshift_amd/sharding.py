"""Data-parallel plumbing: one process per GPU, images are independent units.

The reference shards every loader batch by rank (sampler.py:273-277: `micro = ceil(bs / num_gpus)`,
slice `[rank*micro, (rank+1)*micro)`) and issues no data collective — only barriers (sampler.py:234,291);
every rank re-reads the checkpoint itself (sampler.py:108-112).  Here rank 0 reads and packs the weights
once and the packed blob travels to the other GPUs in ONE RCCL broadcast over xGMI
(`torch.distributed` backend "nccl" is RCCL on ROCm).  Steady state has zero collectives.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _lib


def free_port() -> int:
    """A TCP port that is free on 127.0.0.1 right now (taken from a bound socket, so two launches on one node do not collide
    on a fixed rendezvous port)."""
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return int(s.getsockname()[1])


def pick_backend(world: int) -> str:
    """RCCL ("nccl" on ROCm) when every rank has its own GPU.  Several ranks on one GPU is a plumbing-test configuration only:
    it has to be asked for with RESSHIFT_DIST_BACKEND=gloo, otherwise the launch is refused (RCCL cannot put two ranks on one
    device, and a silent fallback would report a one-GPU number as a multi-GPU one)."""
    forced = os.environ.get("RESSHIFT_DIST_BACKEND")
    if forced:
        return forced
    if not torch.cuda.is_available():
        return "gloo"
    if torch.cuda.device_count() < world:
        raise RuntimeError(f"{world} ranks requested but only {torch.cuda.device_count()} GPU(s) are visible: one process per GPU over "
                           f"RCCL needs {world} devices (set RESSHIFT_DIST_BACKEND=gloo to let the ranks share a GPU for a plumbing test)")
    return "nccl"


def launch_command(script: str, script_args: Sequence[str], nproc: int) -> list:
    """`python -m torch.distributed.run` command line that runs `script` as `nproc` ranks of one node (one process per GPU,
    sampler.py:66-77), rendezvous on 127.0.0.1 at a free port."""
    import sys

    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
            "--master-port", str(free_port()), script, *script_args]


def init_distributed() -> Tuple[int, int]:
    """Returns (world_size, rank).  Initialises the process group from the torchrun environment when WORLD_SIZE > 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    backend = pick_backend(world) if world > 1 else None
    if torch.cuda.is_available():
        # RCCL: rank <-> device is one to one, LOCAL_RANK IS the device (a modulo would silently put two ranks on one GPU and RCCL would
        # hang or fail much later); only the gloo plumbing configuration (several ranks sharing a GPU on purpose) wraps around
        ndev = torch.cuda.device_count()
        if backend == "nccl" and local >= ndev:
            raise RuntimeError(f"LOCAL_RANK {local} has no GPU of its own ({ndev} visible): one process per GPU over RCCL")
        torch.cuda.set_device(local if backend == "nccl" else local % max(1, ndev))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        # RCCL ("nccl") with one GPU per rank; RESSHIFT_DIST_BACKEND=gloo lets several ranks share one GPU for plumbing tests
        kw = {}
        if backend == "nccl":   # bind the communicator to this rank's device up front (no lazy device guess at the first collective)
            kw["device_id"] = torch.device("cuda", torch.cuda.current_device())
        # (gloo / RCCL print connection banners from C++ straight to fd 1; a caller's stdout may be a protocol - bench.py's is ONE JSON line -
        # so fd 1 points at stderr while the communicator comes up)
        import sys

        sys.stdout.flush()
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            dist.init_process_group(backend=backend, init_method="env://", rank=rank, world_size=world, **kw)
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
    return world, rank


def dist_info() -> dict:
    """what bench.py prints about the process group: backend, world size, this rank's device, the RCCL version when the backend is RCCL"""
    info = {"world_size": dist.get_world_size() if dist.is_initialized() else 1, "backend": dist.get_backend() if dist.is_initialized() else None,
            "device": torch.cuda.current_device() if torch.cuda.is_available() else None, "rccl_version": None}
    if info["backend"] == "nccl":
        try:
            info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:   # informational only
            pass
    return info


def allgather_floats(values: Sequence[float], device) -> list:
    """[world][len(values)] python floats: every rank's `values` (bench: per-rank times)."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return [list(values)]
    t = torch.tensor(list(values), dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else device)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    return [[float(v) for v in p.cpu()] for p in parts]


def barrier() -> None:
    """sampler.py:234,291.  Under RCCL the barrier is told its device: without `device_ids` torch guesses the device from the global rank
    (a warning, and the wrong GPU whenever rank != device)."""
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend() == "nccl":
            dist.barrier(device_ids=[torch.cuda.current_device()])
        else:
            dist.barrier()


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous per-rank slice of a batch of n units (sampler.py:273-277); trailing ranks may be empty."""
    micro = math.ceil(n / max(1, world))
    lo = min(n, rank * micro)
    return lo, min(n, lo + micro)


def shard_batch(t: torch.Tensor, rank: int, world: int, dim: int = 0) -> torch.Tensor:
    lo, hi = shard_bounds(t.shape[dim], rank, world)
    return t.narrow(dim, lo, hi - lo)


def shard_noise(noise: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """noise: [steps+1, B_global, C, h, w] drawn for the FULL batch; a sample's noise depends on its position in
    the global batch, so every rank slices the same global tensor (parity with a single-GPU run)."""
    return shard_batch(noise, rank, world, dim=1).contiguous()


def broadcast_blob(blob: torch.Tensor, src: int = 0) -> torch.Tensor:
    """One collective for the whole packed weight blob (flat uint8 tensor)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if blob.is_cuda and dist.get_backend() == "gloo":  # test-only path: stage through the host
            host = blob.cpu()
            dist.broadcast(host, src=src)
            blob.copy_(host)
        else:
            dist.broadcast(blob, src=src)
    return blob


def allreduce_max(value: float, device) -> float:
    """max over ranks of a python float (bench timing)."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return value
    t = torch.tensor([value], dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_images(local: torch.Tensor, n_global: int, rank: int, world: int) -> torch.Tensor:
    """Collect per-rank outputs on every rank in global batch order (host-side convenience, not on the hot path)."""
    if world == 1 or not (dist.is_available() and dist.is_initialized()):
        return local
    micro = math.ceil(n_global / world)
    pad = torch.zeros((micro,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat(parts, 0)[:n_global]


def reflect_pad(x: torch.Tensor, pad_h: int, pad_w: int) -> torch.Tensor:
    """F.pad(..., mode='reflect') on the bottom/right (sampler.py:130-138), on the device (rs_window_copy)."""
    H, W = x.shape[-2:]
    if pad_h >= H or pad_w >= W:
        raise ValueError("reflect padding must be smaller than the padded side (as torch.nn.functional.pad requires)")
    return _lib.window_copy(x, 0, 0, H + pad_h, W + pad_w)


BLOB_CACHE_MAGIC = b"RSBLOB06"   # bump when the packed layout (csrc/model.hip, csrc/weight_pack.h) changes
BLOB_CACHE_HEADER = 40            # magic 8 | blob bytes 8 | checkpoint fingerprint 16 | packed weight forms 4 | reserved 4


def checkpoint_fingerprint(paths) -> bytes:
    """16 bytes identifying the checkpoint files a blob was packed from (path, size, mtime): two checkpoints of one
    architecture (realsr v1 / v2, a retrained ckpt_path) give the same blob size, so the size alone cannot tell a stale cache."""
    import hashlib

    h = hashlib.sha256()
    for p in paths or ():
        if p is None:
            h.update(b"<none>")
            continue
        p = os.path.abspath(str(p))
        h.update(p.encode())
        try:
            st = os.stat(p)
            h.update(f"{st.st_size}:{st.st_mtime_ns}".encode())
        except OSError:
            h.update(b"<missing>")
    return h.digest()[:16]


def _forms_word(eng) -> bytes:
    """which weight forms the engine packs (bit 0 fp16, 1 fp32, 2 split storage): two precision policies sharing one cache path must not
    mistake each other's blob for their own on the strength of a coinciding byte count"""
    cfg = getattr(eng, "cfg", None)
    if cfg is None:
        return (0xFFFFFFFF).to_bytes(4, "little")
    return (int(bool(cfg.enable_f16)) | int(bool(cfg.enable_f32)) << 1 | int(bool(cfg.enable_split)) << 2).to_bytes(4, "little")


def _blob_cache_load(path, eng, fingerprint: bytes = b"\0" * 16) -> bool:
    """Fill the engine's device blob from a packed-blob cache file; False when absent / stale (magic, size, the fingerprint
    of the checkpoints it was packed from, or the set of weight forms that was packed)."""
    if not path or not os.path.exists(path):
        return False
    blob = eng.weight_blob()
    with open(path, "rb") as fh:
        head = fh.read(BLOB_CACHE_HEADER)
        if (len(head) != BLOB_CACHE_HEADER or head[:8] != BLOB_CACHE_MAGIC or int.from_bytes(head[8:16], "little") != blob.numel()
                or head[16:32] != fingerprint or head[32:36] != _forms_word(eng)):
            return False
        import numpy as np

        data = np.fromfile(fh, dtype=np.uint8, count=blob.numel())
    if data.size != blob.numel():
        return False
    blob.copy_(torch.from_numpy(data))
    return True


def _blob_cache_save(path, eng, fingerprint: bytes = b"\0" * 16) -> None:
    blob = eng.weight_blob().cpu().numpy()
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "wb") as fh:
        fh.write(BLOB_CACHE_MAGIC + int(blob.size).to_bytes(8, "little") + fingerprint + _forms_word(eng) + b"\0" * 4)
        blob.tofile(fh)
    os.replace(tmp, path)


def weight_forms(precisions) -> dict:
    """Engine(enable_f16 / enable_f32 / enable_split) flags for the storage types a run will ask for.  `precisions`: None (all three
    forms: a process that switches policies at will, e.g. the test-suite) or an iterable of precision names ("fp16", "fp32", "split" and
    their aliases) - the engine then packs, broadcasts and caches only those forms of every conv / linear weight (a parity-policy
    run: split for the encoder + UNet, fp16 for the decoder - no fp32 copy), and a later call that names another precision fails loudly."""
    if precisions is None:
        return dict(enable_f16=True, enable_f32=True, enable_split=True)
    from .engine import F16, F32, SPLIT, parse_precision

    want = {parse_precision(p) for p in precisions}
    return dict(enable_f16=F16 in want, enable_f32=F32 in want, enable_split=SPLIT in want)


def build_engine_with_broadcast(model, autoencoder, load_fn: Callable[[], Sequence], rank: int, world: int, blob_cache=None,
                                cache_fingerprint: bytes = b"\0" * 16, precisions=None):
    """Create the fused UNet+AE engine on this rank's GPU.  Rank 0 calls `load_fn()` -> (unet_sd, ae_sd), fills the
    drop-in modules (reload_model semantics) and packs the device blob; the blob is then broadcast.

    `blob_cache`: path of a packed-blob file.  When it exists (and matches this configuration's blob size and
    `cache_fingerprint`, see checkpoint_fingerprint) rank 0 uploads
    it instead of reading and repacking the checkpoints - the drop-in modules then keep their initial parameters, only
    the engine owns the real weights; otherwise the freshly packed blob is written there for the next start."""
    from .engine import Engine
    from .sampler import reload_model

    dev = next(model.parameters()).device
    eng = Engine(unet_params=model.params, ae_params=autoencoder.params, device=dev, **weight_forms(precisions))   # (`precisions`: weight_forms)
    if rank == 0 and not _blob_cache_load(blob_cache, eng, cache_fingerprint):
        unet_sd, ae_sd = load_fn()
        with torch.no_grad():
            reload_model(model, unet_sd)
            reload_model(autoencoder, ae_sd)
        eng.load_state_dicts(unet_sd=model.state_dict(), ae_sd=autoencoder.state_dict())
        eng._packed_from_modules = True
        if blob_cache:
            torch.cuda.synchronize(dev)
            _blob_cache_save(blob_cache, eng, cache_fingerprint)
    eng.broadcast_s, eng.broadcast_bytes = 0.0, 0
    if world > 1:
        import time

        torch.cuda.synchronize(dev)
        barrier()
        t0 = time.perf_counter()
        broadcast_blob(eng.weight_blob(), src=0)
        torch.cuda.synchronize(dev)
        eng.broadcast_s, eng.broadcast_bytes = time.perf_counter() - t0, int(eng.weight_blob().numel())
    eng.mark_weights_ready()
    # the module shells hand out THIS engine from now on (model(x, t), encode / decode, the step-wise sampling API): on ranks
    # other than 0, and on rank 0 after a blob-cache hit, their own parameters were never filled - an engine rebuilt from
    # them would compute on zeros.  (`state_dict()` of such a shell is NOT the checkpoint; only the engine owns the weights.)
    from .unet import params_version

    for m in (model, autoencoder):
        m._engine, m._engine_version = eng, params_version(m)
    model.weights_in_engine_only = autoencoder.weights_in_engine_only = not (rank == 0 and getattr(eng, "_packed_from_modules", False))
    return eng
