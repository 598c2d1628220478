"""ORACLE support — test infrastructure only (see resshift_oracle.py header).

Deterministic synthetic weights and inputs.  The released ResShift checkpoints cannot be fetched
(no network) and the reference zero-initialises 167 tensors (models/unet.py:172-174,
models/basic_ops.py:64-70), so parity runs re-randomise EVERY tensor.  Values come from numpy's
PCG64 seeded per tensor name, hence are identical on any machine and independent of key order.
regime_state_dict derives further weight regimes from that draw (quiet, loud, and the reference's
zero-initialised state), so that the block tests do not all sit in one operand range.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict
from typing import Dict, Iterable, Tuple

import numpy as np
import torch

from . import resshift_oracle as oc


def _rng(seed: int, name: str) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))


def synthetic_state_dict(spec: "Dict[str, Tuple[int, ...]]", seed: int, image_size: int = 64, window: int = 8) -> "OrderedDict[str, torch.Tensor]":
    """spec: key -> shape in the reference's state_dict naming (resshift_amd.spec builds it; tests pass it in)."""
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in spec.items():
        g = _rng(seed, name)
        if name.endswith("relative_position_index"):
            sd[name] = oc._rel_index(window)
            continue
        if name.endswith("attn_mask"):
            n_w = shape[0]
            side = int(round(n_w ** 0.5)) * window
            sd[name] = oc._shift_mask(side, side, window, window // 2)
            continue
        x = g.standard_normal(shape, dtype=np.float32)
        if name.endswith("relative_position_bias_table"):
            x *= 0.5
        elif name == "quantize.embedding.weight":
            x *= 0.6
        elif len(shape) == 1 and name.endswith(".weight"):  # GroupNorm gains
            x = 1.0 + 0.1 * x
        elif len(shape) == 1:  # biases (conv / linear / GroupNorm)
            x *= 0.05
        else:  # conv / linear weights: fan-in scaled
            fan_in = int(np.prod(shape[1:]))
            x *= 1.0 / np.sqrt(fan_in)
            if ".emb_layers." in name:
                x *= 0.5
            if name == "decoder.conv_out.weight":
                x *= 0.3  # keep most decoded pixels inside [-1,1] so that PSNR on the clamped image is meaningful
        sd[name] = torch.from_numpy(np.ascontiguousarray(x))
    return sd


REGIMES = ("quiet", "loud", "zero_init")
# the factors of the "loud" regime (see regime_state_dict)
LOUD = {"bias": 20.0, "gain_spread": 5.0, "table": 8.0, "qkv": 3.0, "fc1": 4.0, "emb": 4.0, "ae_qk": 4.0}


def zero_module_names(names: Iterable[str]):
    """The tensors the reference passes through zero_module (models/unet.py:172, :970): weight and bias of every ResBlock's second
    conv (out_layers.3) and of the output head's conv (out.2), picked from key names in resshift_amd.spec's naming."""
    names = list(names)
    res = sorted({n[: -len(".in_layers.0.weight")] for n in names if n.endswith(".in_layers.0.weight")})   # every ResBlock of the spec
    want = [f"{r}.out_layers.3.{s}" for r in res for s in ("weight", "bias")]
    if "out.0.weight" in names:
        want += ["out.2.weight", "out.2.bias"]
    assert all(n in names for n in want), [n for n in want if n not in names]
    return want


def regime_state_dict(sd: "Dict[str, torch.Tensor]", kind: str) -> "OrderedDict[str, torch.Tensor]":
    """A second weight regime from a synthetic state dict (UNet or autoencoder): a pure function of `sd`, which is left alone.  Index and
    mask buffers and the codebook pass through untouched; "weights" are tensors with ndim >= 2 that are not a bias table, "biases" the
    1-D tensors that are not GroupNorm gains (conv, linear and GroupNorm biases alike).

    "quiet": every conv / linear weight and every bias x 0.01, except quant_conv / post_quant_conv: GroupNorm inputs whose variance is
        of the order of eps or far below it (tests/test_unet_blocks_cpu.py, test_ae_blocks_cpu.py pin the ranges).
    "loud": biases x 20, GroupNorm gains spread x 5 (1 + 5 (g - 1)), relative position bias table x 8, .attn.qkv. weights x 3,
        .mlp.fc1. weights x 4, .emb_layers. weights x 4, {encoder,decoder}.mid.attn_1.{q,k} weights x 4 (the factors: LOUD); every
        other weight as it is.  Peaked softmaxes, GELU arguments up to 30, SiLU arguments far out on both sides.
    "zero_init": the tensors the reference's zero_module touches (zero_module_names) exactly zero, everything else as it is: the
        reference's own initial state."""
    if kind not in REGIMES:
        raise ValueError(f"unknown regime {kind!r}")
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    zero = set(zero_module_names(sd.keys())) if kind == "zero_init" else set()
    for name, v in sd.items():
        if (not torch.is_floating_point(v)) or name.endswith("attn_mask") or name == "quantize.embedding.weight":
            out[name] = v.clone()
            continue
        table = name.endswith("relative_position_bias_table")
        gain = v.ndim == 1 and name.endswith(".weight")
        bias = v.ndim == 1 and not gain
        weight = v.ndim >= 2 and not table
        f = 1.0
        if kind == "quiet":
            if (weight or bias) and not name.startswith(("quant_conv.", "post_quant_conv.")):
                f = 0.01
        elif kind == "loud":
            if bias:
                f = LOUD["bias"]
            elif table:
                f = LOUD["table"]
            elif weight and ".attn.qkv." in name:
                f = LOUD["qkv"]
            elif weight and ".mlp.fc1." in name:
                f = LOUD["fc1"]
            elif weight and ".emb_layers." in name:
                f = LOUD["emb"]
            elif weight and name in tuple(f"{p}.mid.attn_1.{s}.weight" for p in ("encoder", "decoder") for s in ("q", "k")):
                f = LOUD["ae_qk"]
        if kind == "loud" and gain:
            out[name] = 1.0 + LOUD["gain_spread"] * (v - 1.0)
        elif name in zero:
            out[name] = torch.zeros_like(v)
        else:
            out[name] = v * f if f != 1.0 else v.clone()
    return out


def synthetic_inputs(seed: int, B: int, h: int, w: int, cz: int, hz: int, wz: int, steps: int, with_mask: bool = False):
    """LR batch in [-1,1], the (steps+1) noise tensors in draw order, and an optional inpainting mask."""
    g = _rng(seed, "inputs")
    y = torch.from_numpy(g.random((B, 3, h, w), dtype=np.float32) * 2 - 1)
    noises = [torch.from_numpy(g.standard_normal((B, cz, hz, wz), dtype=np.float32)) for _ in range(steps + 1)]
    mask = None
    if with_mask:
        mask = torch.from_numpy(((g.random((B, 1, h, w), dtype=np.float32) > 0.7).astype(np.float32)) * 2 - 1)
    return y, noises, mask
