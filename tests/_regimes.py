"""Shared by the weight-regime tests (test_unet_blocks_*.py, test_ae_blocks_*.py): the regime weights, the inputs of the regime cases, a
probe of what a regime exercises (GroupNorm var / eps and |mean| / std per group, the largest softmax probability per row, GELU arguments,
conv outputs) and the float32 oracle's own error on a teacher-forced plan step - the yardstick the regime tolerances scale with."""
import contextlib

import torch
import torch.nn.functional as F

import helpers as H

REGIMES = H.synth.REGIMES
# tolerance of a block = max(TOL[prec], K32[prec] * err32), err32 = the float32 oracle's error on the same teacher-forced inputs: 4 for fp32
# storage (another summation order, x 2 margin), 8 for split (the pair keeps 2^-22 of an operand, 4 x fp32's unit, x 2 margin); fp16 storage
# keeps its fixed tolerance
K32 = {"fp32": 4.0, "split": 8.0}
ERR32_CAP = 1e-4   # what the yardstick itself may be, on every block of every regime case (asserted on the CPU)


def regime_sd(sd, regime):
    """the synthetic state dict in a regime ("base": as it is)"""
    return sd if regime == "base" else H.synth.regime_state_dict(sd, regime)


def unet_case_inputs(up, B, h, w, T, ts="mixed"):
    """(x, lq, mask, t) of a case of tests/test_unet_blocks_gpu.py"""
    hz, hl = int(up["image_size"]), int(up["lq_size"])
    lh, lw = h * hl // hz, w * hl // hz
    g = torch.Generator().manual_seed(1000 + B)
    x = torch.randn(B, int(up["in_channels"]), h, w, generator=g)
    lq = torch.rand(B, 3, lh, lw, generator=g) * 2 - 1
    mask = ((torch.rand(B, 1, lh, lw, generator=g) > 0.6).float() * 2 - 1) if up.get("cond_mask") else None
    t = [(7 * b) % T for b in range(B)] if ts == "mixed" else [7 % T] * B
    return x, lq, mask, t


def ae_case_inputs(ap, call, B, h, w):
    """the image (encode) or the latent (decode) of a case of tests/test_ae_blocks_gpu.py"""
    if call == "encode":
        return torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(1000 + B)) * 2 - 1
    return H.vq_latents(B, int(ap["embed_dim"]), h, w, 2000 + B)


def unet_identity_step(step, sd):
    """a step of oracle.unet_plan that is one ResBlock without a skip conv: with the zero_init weights it returns its first input"""
    n = step.name
    if len(step.inputs) != 2 or step.inputs[1] != "emb":
        return False
    if n.startswith("in."):
        key = f"input_blocks.{n.split('.')[1]}.0"
    elif n in ("mid.res1", "mid.res2"):
        key = "middle_block.0" if n == "mid.res1" else "middle_block.2"
    else:
        return False
    return key + ".in_layers.0.weight" in sd and key + ".skip_connection.weight" not in sd


def per_image_err(got, ref):
    """max |got - ref| / max |ref| per image -> list of floats"""
    return [((got[k].double() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30)).item() for k in range(ref.shape[0])]


def err32(step32, ins, ref64):
    """the float32 oracle's own error on one plan step, per image: `step32` is the step of a plan built on the float32 weights, `ins` the
    teacher-forced inputs the float64 step got (used in float32), `ref64` that float64 step's output.  The reference's own arithmetic,
    never the engine's."""
    return per_image_err(step32.fn(*[v.float() if torch.is_floating_point(v) else v for v in ins]), ref64)


class Probe:
    def __init__(self):
        self.var_eps, self.offcentre, self.pmax, self.gelu, self.conv, self.finite = [], [], [], 0.0, 0.0, True

    def median_var_eps(self):
        return torch.cat(self.var_eps).median().item()

    def min_var_eps(self):
        return torch.cat(self.var_eps).min().item()

    def max_offcentre(self):
        return max(self.offcentre)

    def median_pmax(self):
        return torch.cat(self.pmax).median().item()


@contextlib.contextmanager
def probe():
    """record, while the oracle runs inside: var / eps and |mean| / std of every GroupNorm group, the largest probability of every softmax
    row, the largest |GELU argument| and |conv output|, and whether all of those were finite"""
    p = Probe()
    gn, conv, gelu, fsm, tsm = F.group_norm, F.conv2d, F.gelu, F.softmax, torch.Tensor.softmax

    def _gn(x, groups, weight=None, bias=None, eps=1e-5):
        v = x.double().reshape(x.shape[0], groups, -1)
        var, mean = v.var(dim=2, unbiased=False), v.mean(dim=2)
        p.var_eps.append((var / eps).reshape(-1))
        p.offcentre.append((mean.abs() / var.sqrt().clamp_min(1e-300)).max().item())
        p.finite &= bool(torch.isfinite(x).all())
        return gn(x, groups, weight, bias, eps)

    def _conv(x, *a, **k):
        y = conv(x, *a, **k)
        p.conv = max(p.conv, y.abs().max().item())
        p.finite &= bool(torch.isfinite(y).all())
        return y

    def _gelu(x, *a, **k):
        p.gelu = max(p.gelu, x.abs().max().item())
        return gelu(x, *a, **k)

    def _note(y, dim):
        p.pmax.append(y.amax(dim=dim).reshape(-1).double())
        p.finite &= bool(torch.isfinite(y).all())
        return y

    def _fsm(x, dim=None, **k):
        return _note(fsm(x, dim=dim, **k), dim)

    def _tsm(x, dim=None, **k):
        return _note(tsm(x, dim=dim, **k), dim)

    F.group_norm, F.conv2d, F.gelu, F.softmax, torch.Tensor.softmax = _gn, _conv, _gelu, _fsm, _tsm
    try:
        yield p
    finally:
        F.group_norm, F.conv2d, F.gelu, F.softmax, torch.Tensor.softmax = gn, conv, gelu, fsm, tsm
