"""Shared by tests/test_structures_cpu.py and tests/test_structures_gpu.py: the cases run on the network structures of oracle/cases.py:
STRUCTURES (what each structure is there for is said there), their weights and inputs.  The CPU module walks every case of the GPU module
on the fake device first, so that a planning error shows without a GPU."""
import numpy as np
import torch

import helpers as H
from oracle import cases

S = cases.STRUCTURES
PRECS = {"fp16": 0, "fp32": 1, "split": 2}   # the engine's precision codes (resshift_amd.engine.PRECISIONS)
BIG = ("heads6_mc128", "heads6_mc192")
# the smallest batch that gives the 32 x 32 level of the heads6_* structures the 16384 tokens the fused Swin MLP wants in a launch
B_FUSED = 16

# UNet: (tag, batch, latent h, w - None: the constructed size -, storage).  The small structures run at B = 3 in every storage; the two
# heads6_* ones at B_FUSED in every storage, and at B = 2 in split storage (fused attention beside the two-GEMM MLP, which B_FUSED replaces
# at the top level).  three_uneven also runs a non-square plane: 64 x 32, the smallest its three levels and 8-pixel windows allow - on 32 x 16
# the coarsest level would be 8 x 4, under one window, which the reference's own window partition cannot run either.
UNET = ([(tag, 3, None, None, prec) for tag in S["unet"] if tag not in BIG for prec in ("split", "fp16", "fp32")] +
        [("three_uneven", 2, 64, 32, "split")] +
        [(tag, B_FUSED, None, None, prec) for tag in BIG for prec in ("split", "fp16", "fp32")] +
        [(tag, 2, None, None, "split") for tag in BIG])
# autoencoder: image side of the encode case; the decode case takes the latent it encodes to.  ae_f8_equal at 128: a 16 x 16 latent, 512
# positions for the D = 4 VQ search
AE_SIDE = {"ae_f1": 16, "ae_f8_equal": 128, "ae_f2_wide": 32}
AE = [(tag, call, 2, prec) for tag in S["ae"] for call in ("encode", "decode") for prec in ("split", "fp16", "fp32")]
PAIRS = [(tag, 2, prec) for tag in S["pairs"] for prec in ("split", "fp16", "fp32")]


def ae_factor(ap):
    return 2 ** (len(ap["ddconfig"]["ch_mult"]) - 1)


def ae_plane(tag, call):
    """(h, w) of an autoencoder case: the image (encode) or the latent (decode)"""
    side = AE_SIDE[tag] // (1 if call == "encode" else ae_factor(S["ae"][tag]))
    return side, side


def fake_args(family, tag):
    """the cases of one structure as arguments of tests/_fake_device_structures.py: every case of the GPU module, and B = 2 in every storage"""
    if family == "unet":
        rows = [(B, h, w, p) for t, B, h, w, p in UNET if t == tag] + [(2, None, None, p) for p in PRECS]
        return list(dict.fromkeys(f"unet:{tag}:{B}:{PRECS[p]}" + (f":{h}x{w}" if h else "") for B, h, w, p in rows))
    if family == "ae":
        return ["%s:%s:%d:%d:%dx%d" % ((call, tag, B, PRECS[p]) + ae_plane(tag, call)) for t, call, B, p in AE if t == tag]
    return [f"sample:{tag}:{B}:{PRECS[p]}" for t, B, p in PAIRS if t == tag]


def unet_weights(up):
    return H.synth.synthetic_state_dict(H.unet_param_spec(up)[0], H.SEED_W, image_size=up["image_size"])


def ae_weights(ap):
    return H.synth.synthetic_state_dict(H.ae_param_spec(ap), H.SEED_W)


def fixture():
    from oracle import make_golden_structures as ms

    return np.load(ms.PATH)


def double(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
