"""Helper of tests/test_noise_cpu.py: rs_sample_step and rs_sample_step_seeded under RS_FAKE_DEVICE=1 (test-hooks library; every launch fails,
the bookkeeping of the dry and the real pass does not - see _fake_device_plumbing.py and _fake_device_step.py).  Runs the realsr config's
step at batch B four times - tensor and seeded, every image at one step index and each at its own - printing the engine's "[fake device]"
line of each call on stderr and "CALL <name> rc <rc> launches <n>" on stdout, then one line per argument error of the seeded call:
"ERR <case> rc <rc> <message>".  Usage: _fake_device_step_seeded.py <batch> <precision 0 fp16 | 1 fp32 | 2 split>"""
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

cfgy = to_plain(load_config("realsr_swinunet_realesrgan256"))
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
a.B, a.h, a.w, a.sf = B, 64, 64, int(d.sf)
a.steps = len(tables["coef1"])
for t in range(a.steps):
    a.inv_std[t], a.coef1[t], a.coef2[t], a.sigma[t] = (float(tables[k][t]) for k in ("inv_std", "coef1", "coef2", "sigma"))
    a.tmap[t] = int(tables["tmap"][t])
    a.prec_unet[t] = prec
a.prior_scale, a.scale_factor = float(tables["prior_scale"]), float(d.scale_factor)


def step(ts, keys=None, seeded=False, nb=None, noise=4096):
    s = _lib.StepArgs()
    s.sched = C.pointer(a)
    s.x, s.y, s.noise, s.mask = 4096, 4096, noise, None
    s.B = len(ts) if nb is None else nb
    s.t = (C.c_int * len(ts))(*ts)
    s.prec = prec
    if not seeded:
        return lib.rs_sample_step(h, C.byref(s))
    return lib.rs_sample_step_seeded(h, C.byref(s), keys)


good = _lib.noise_keys([(1000 + b, b % 3) for b in range(B)])
uniform, mixed = [7] * B, [(b * 5) % a.steps for b in range(B)]
for name, ts, seeded in (("tensor_uniform", uniform, False), ("seeded_uniform", uniform, True), ("tensor_mixed", mixed, False),
                         ("seeded_mixed", mixed, True)):
    rc = step(ts, good, seeded, noise=None if seeded else 4096)   # (the seeded call ignores the noise member)
    sys.stderr.flush()
    print(f"CALL {name} rc {rc} launches {lib.rs_last_launch_count(h)}", flush=True)
bad = _lib.noise_keys([(1, 0)] * B)
bad[B - 1].reserved = 1
many = _lib.noise_keys([(b, 0) for b in range(_lib.RS_MAX_ROWS + 1)])
errors = {
    "null_keys": lambda: step(uniform, None, True),
    "reserved": lambda: step(uniform, bad, True),
    "b_zero": lambda: step(uniform, good, True, nb=0),
    "b_bound_mixed": lambda: step([b % 2 for b in range(_lib.RS_MAX_ROWS + 1)], many, True),
    "tensor_null_noise": lambda: step([3] * B, None, False, noise=None),
}
for name, fn in errors.items():
    rc = fn()
    print(f"ERR {name} rc {rc} {_lib.last_error()}", flush=True)
