"""Helper of tests/test_continuous_cpu.py: rs_sample_step under RS_FAKE_DEVICE=1 (test-hooks library; every launch fails, the bookkeeping of the
dry and the real pass does not - see _fake_device_plumbing.py).  Runs the realsr config's step at batch B twice - every image at one step
index, then each at its own - and prints the engine's "[fake device]" line of each call on stderr, then one line per argument error:
"ERR <case> rc <rc> <message>".  Usage: _fake_device_step.py <batch> <precision 0 fp16 | 1 fp32 | 2 split>"""
import ctypes as C
import os
import sys

os.environ["RS_FAKE_DEVICE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from resshift_amd import _lib  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.engine import _fill_ae, _fill_unet  # noqa: E402
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion  # noqa: E402

lib = _lib.load()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
prec = int(sys.argv[2]) if len(sys.argv) > 2 else 2


def engine(cname, lr):
    cfgy = to_plain(load_config(cname))
    up, aep, dp = cfgy["model"]["params"], cfgy["autoencoder"]["params"], cfgy["diffusion"]["params"]
    cfg = _lib.Config()
    _fill_unet(cfg.unet, up)
    cfg.has_unet = 1
    _fill_ae(cfg.ae, aep)
    cfg.has_ae = 1
    cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
    h = lib.rs_create(C.byref(cfg))
    assert h
    lib.rs_bind_weight_blob(h, 256 * 1024, lib.rs_weight_bytes(h))   # fake, aligned address: never dereferenced on the host
    assert lib.rs_weights_ready(h) == 0
    d = create_gaussian_diffusion(**dp)
    tables = d.step_tables()
    a = _lib.SampleArgs()
    a.B, a.h, a.w, a.sf = B, lr, lr, int(d.sf)
    a.steps = len(tables["coef1"])
    for t in range(a.steps):
        a.inv_std[t], a.coef1[t], a.coef2[t], a.sigma[t] = (float(tables[k][t]) for k in ("inv_std", "coef1", "coef2", "sigma"))
        a.tmap[t] = int(tables["tmap"][t])
        a.prec_unet[t] = prec
    a.prior_scale, a.scale_factor = float(tables["prior_scale"]), float(d.scale_factor)
    return h, a


def step(h, a, ts, nb=None, x=4096, noise=4096, mask=None):
    s = _lib.StepArgs()
    s.sched = C.pointer(a)
    s.x, s.y, s.noise, s.mask = x, 4096, noise, mask
    s.B = len(ts) if nb is None else nb
    s.t = (C.c_int * len(ts))(*ts)
    s.prec = prec
    return lib.rs_sample_step(h, C.byref(s))


h, a = engine("realsr_swinunet_realesrgan256", 64)
for name, ts in (("uniform", [7] * B), ("mixed", [(b * 5) % a.steps for b in range(B)])):
    rc = step(h, a, ts)
    sys.stderr.flush()
    print(f"CALL {name} rc {rc} launches {lib.rs_last_launch_count(h)}", flush=True)
errors = {
    "t_range": lambda: step(h, a, [0] * (B - 1) + [a.steps]),
    "t_negative": lambda: step(h, a, [-1] + [0] * (B - 1)),
    "b_bound": lambda: step(h, a, [b % 2 for b in range(_lib.RS_MAX_ROWS + 1)]),
    "null_x": lambda: step(h, a, [3] * B, x=None),
    "null_noise": lambda: step(h, a, [3] * B, noise=None),
}
hm, am = engine("inpaint_lama256_imagenet", 256)
errors["no_mask"] = lambda: step(hm, am, [3] * B)
for name, fn in errors.items():
    rc = fn()
    print(f"ERR {name} rc {rc} {_lib.last_error()}", flush=True)
