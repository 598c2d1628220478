"""Every UNet block of the production kernel graph against float64, teacher-forced, per image.

The engine runs its own kernel choice at each batch (Winograd on the 64 x 64 / 32 x 32 levels at the bench batch, split-K small-plane
halo kernels, GroupNorm tails and folds, fused qkv attention, the fused Swin MLP with the patch-unembed fold, the shortcut fold, the
sub-pixel upsampling conv, the fused head, a per-image FiLM table at mixed timesteps).  A traced call (Engine.debug_enable) runs that same
graph - the test asserts it: same output bits, same launch count - and records every block boundary.  Each block of the plan
(oracle/resshift_oracle.py: unet_plan) is then fed the engine's own recorded inputs in float64 and compared with the engine's output of
that block, per image: max |engine - ref| / max |ref| over the image's block output, so that one image reading another image's FiLM row
cannot hide behind another image's scale, and errors do not build up along the chain.  Run with -s for the table of the worst error per
block and precision (the margin later kernel changes have left)."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import resshift_oracle as oc
from resshift_amd.config import load_config, to_plain
from resshift_amd.engine import Engine, parse_precision
from resshift_amd.spec import unet_param_spec

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CONFIGS = {"realsr": "realsr_swinunet_realesrgan256", "faceir": "faceir_gfpgan512_lpips", "inpaint": "inpaint_lama256_imagenet"}
CASES = [("realsr", 32, "split", "mixed"), ("realsr", 32, "fp16", "mixed"), ("realsr", 32, "fp32", "mixed"), ("realsr", 32, "split", "shared"),
         ("realsr", 3, "split", "mixed"), ("realsr", 3, "fp16", "mixed"), ("realsr", 3, "fp32", "mixed"),
         ("faceir", 16, "split", "mixed"), ("faceir", 16, "fp16", "mixed"), ("inpaint", 16, "split", "mixed"), ("inpaint", 16, "fp16", "mixed")]
# Per-image tolerance of every block, per precision: under 3x the worst error measured over all CASES on the MI355X.  Measured (worst
# block): split 1.79e-6 (head; the upsampling convs out.2 / out.5 1.4e-6 / 1.0e-6, every other block <= 1.2e-6), fp16 8.8e-4 (in.1, fp16
# storage of the block output), fp32 3.6e-6 (the upsampling convs out.2 / out.5 / out.8: 3.6e-6 / 2.7e-6 / 3.2e-6 - K = 9 x 640 products
# in one fp32 sum -, every other block <= 1.9e-6).
TOL = {"split": 5e-6, "fp16": 2.5e-3, "fp32": 1e-5}

_models = {}
_worst = {}   # (block, prec) -> worst per-image error over the cases run so far


@pytest.fixture(scope="module", autouse=True)
def _table():
    """after the module: the table of the worst per-image error per block and precision over every case that ran (-s)"""
    yield
    if not _worst:
        return
    precs = [p for p in TOL if any(pp == p for _, pp in _worst)]
    names = list(dict.fromkeys(n for n, _ in _worst))
    print("\nworst per-image error per block (max |engine - float64| / max |float64|, teacher-forced):")
    print(f"{'block':<12}" + "".join(f"{p:>12}" for p in precs))
    for n in names:
        print(f"{n:<12}" + "".join(f"{_worst.get((n, p), float('nan')):>12.3e}" for p in precs))
    print(f"{'worst':<12}" + "".join(f"{max(v for (n, pp), v in _worst.items() if pp == p):>12.3e}" for p in precs))
    print(f"{'tolerance':<12}" + "".join(f"{TOL[p]:>12.1e}" for p in precs))
    _models.clear()


def _model(key, gpu):
    if key not in _models:
        cfg = to_plain(load_config(CONFIGS[key]))
        up, dp = cfg["model"]["params"], cfg["diffusion"]["params"]
        uspec, _ = unet_param_spec(up)
        usd = H.synth.synthetic_state_dict(uspec, H.SEED_W, image_size=up["image_size"])
        sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in usd.items()}
        eng = Engine(unet_params=up, ae_params=None, device=gpu)
        eng.load_state_dicts(unet_sd=usd)
        eng.mark_weights_ready()
        _models[key] = (up, int(dp["steps"]), sd64, eng)
    return _models[key]


def _pick(B):
    """8 images spread over the batch, the first and the last included (all of a smaller batch)"""
    return sorted(set(int(v) for v in np.linspace(0, B - 1, min(8, B)).round()))


@pytest.mark.parametrize("key,B,prec,ts", CASES, ids=[f"{k}-B{b}-{p}-{t}" for k, b, p, t in CASES])
def test_every_unet_block_against_float64(gpu, key, B, prec, ts):
    up, T, sd64, eng = _model(key, gpu)
    hz, hl = int(up["image_size"]), int(up["lq_size"])
    g = torch.Generator().manual_seed(1000 + B)
    x = torch.randn(B, int(up["in_channels"]), hz, hz, generator=g)
    lq = torch.rand(B, 3, hl, hl, generator=g) * 2 - 1
    mask = ((torch.rand(B, 1, hl, hl, generator=g) > 0.6).float() * 2 - 1) if up.get("cond_mask") else None
    t = [(7 * b) % T for b in range(B)] if ts == "mixed" else [7 % T] * B
    args = dict(lq=lq.to(gpu), mask=mask.to(gpu) if mask is not None else None, prec=parse_precision(prec))

    # the same pass untraced and traced: same bits, same network launches
    eng.debug_enable(False)
    out = eng.unet_forward(x.to(gpu), t, **args)
    torch.cuda.synchronize()
    n_plain = eng.last_launch_count()
    eng.debug_enable(True)
    try:
        out_tr = eng.unet_forward(x.to(gpu), t, **args)
        n_traced = eng.last_launch_count()
        fam = {name: n for name, fl, ms, n in eng.profile_families()}
        pick = _pick(B)
        trace = {k: v[pick].double().cpu() for k, v in eng.debug_trace().items()}
    finally:
        eng.debug_enable(False)
    assert torch.equal(out, out_tr), "a traced pass computes something else than an untraced one"
    assert n_plain == n_traced, (n_plain, n_traced)
    if B == 32 and prec == "split":
        nw = [n for name, n in fam.items() if name.startswith("wino_kernel")]
        assert nw and nw[0] >= 10, fam   # the traced bench-batch pass ran the Winograd kernels it is meant to check

    # every block of the plan, teacher-forced, in float64, per image
    host = {"x": x[pick].double(), "t": torch.tensor([t[b] for b in pick]), "lq": lq[pick].double()}
    if mask is not None:
        host["mask"] = mask[pick].double()
    plan = oc.unet_plan(sd64, up, with_lq=True, with_mask=mask is not None)
    got_head = out[pick].double().cpu()
    env = dict(host)
    failures, missing = [], []
    for s in plan:
        if s.name != "emb" and s.name != "head" and s.name not in trace:
            missing.append(s.name)
            continue
        ins = [env[i] if i in env else trace.get(i) for i in s.inputs]
        if any(v is None for v in ins):
            continue   # (an input block is missing: reported above)
        ref = s.fn(*ins)
        if s.name == "emb":
            env["emb"] = ref
            continue
        got = got_head if s.name == "head" else trace[s.name]
        assert got.shape == ref.shape, (s.name, got.shape, ref.shape)
        for k, b in enumerate(pick):
            e = ((got[k] - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30)).item()
            _worst[(s.name, prec)] = max(_worst.get((s.name, prec), 0.0), e)
            if not np.isfinite(e) or e > TOL[prec]:
                failures.append(f"{s.name}: image {b} (t={t[b]}) error {e:.3e} > {TOL[prec]:.1e}")
    worst = max((v for (n, p), v in _worst.items() if p == prec), default=0.0)
    print(f"\n{key} B={B} {prec} {ts}: {len(plan) - 1} blocks x {len(pick)} images, worst {prec} error so far {worst:.3e}")
    assert not missing, f"blocks of the plan missing from the trace: {missing}"
    assert not failures, "\n".join(failures[:40])
