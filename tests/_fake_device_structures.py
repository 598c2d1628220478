"""Helper of tests/test_structures_cpu.py, the sibling of _fake_device_plumbing.py for networks built from oracle/cases.py: STRUCTURES instead
of a YAML name: with RS_FAKE_DEVICE=1 the engine's real pass walks its whole control flow on a host-memory arena while every launch fails,
and prints what the dry sizing pass and the real pass each counted.  One process runs any number of cases, one argument each:

    <call>:<tag>:<batch>:<precision 0 fp16 | 1 fp32 | 2 split>[:<h>x<w>]

call = unet (rs_unet_forward on a UNet structure; h x w: the latent plane, default the constructed one), encode / decode (rs_vq_encode /
rs_vq_decode on an autoencoder structure; h x w: the image / the latent, required) or sample (rs_sample on a pair, at the LR size that
gives the UNet's constructed latent).  Per case: a "case <argument>" line on stderr ahead of the engine's own "[fake device]" lines, then
on stdout "<argument> rc <rc> err <rs_last_error> launches <n> families <per family> igemm <n> gn <n>"."""
import ctypes as C
import os
import sys

os.environ["RS_FAKE_DEVICE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cases  # noqa: E402
from resshift_amd import _lib  # noqa: E402
from resshift_amd.engine import _fill_ae, _fill_unet  # noqa: E402
from resshift_amd.gaussian_diffusion import create_gaussian_diffusion  # noqa: E402

lib = _lib.load()
S = cases.STRUCTURES
FAKE = 4096   # a fake, aligned device address: never dereferenced on the host
_engines = {}


def engine(up, ap, key):
    if key not in _engines:
        cfg = _lib.Config()
        if up is not None:
            _fill_unet(cfg.unet, up)
            cfg.has_unet = 1
        if ap is not None:
            _fill_ae(cfg.ae, ap)
            cfg.has_ae = 1
        cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
        h = lib.rs_create(C.byref(cfg))
        assert h, _lib.last_error()
        lib.rs_bind_weight_blob(h, 256 * 1024, lib.rs_weight_bytes(h))
        assert lib.rs_weights_ready(h) == 0
        _engines[key] = h
    return _engines[key]


def run(arg):
    f = arg.split(":")
    call, tag, B, prec = f[0], f[1], int(f[2]), int(f[3])
    hw = tuple(int(v) for v in f[4].split("x")) if len(f) > 4 else None
    if call == "unet":
        up = S["unet"][tag]
        h = engine(up, None, ("unet", tag))
        hz, hl = int(up["image_size"]), int(up["lq_size"])
        H, W = hw or (hz, hz)
        ts = (C.c_int * B)(*[(7 * b) % 4 for b in range(B)])
        rc = lib.rs_unet_forward(h, FAKE, ts, FAKE, FAKE if up.get("cond_mask") else None, FAKE, B, H, W, H * hl // hz, W * hl // hz, prec, None)
    elif call in ("encode", "decode"):
        h = engine(None, S["ae"][tag], ("ae", tag))
        if call == "encode":
            rc = lib.rs_vq_encode(h, FAKE, FAKE, B, hw[0], hw[1], prec, None)
        else:
            rc = lib.rs_vq_decode(h, FAKE, FAKE, FAKE, B, hw[0], hw[1], 0, prec, None)
    else:
        up, ap, dp, with_mask = cases.structure_pair(tag)
        h = engine(up, ap, ("pair", tag))
        d = create_gaussian_diffusion(**dp)
        tables = d.step_tables()
        steps = len(tables["coef1"])
        a = _lib.SampleArgs()
        a.y = a.noise = a.out = FAKE
        a.mask = FAKE if with_mask else None
        lr = int(up["lq_size"])
        a.B, a.h, a.w, a.sf, a.steps = B, lr, lr, int(d.sf), steps
        for t in range(steps):
            a.inv_std[t], a.coef1[t], a.coef2[t] = float(tables["inv_std"][t]), float(tables["coef1"][t]), float(tables["coef2"][t])
            a.sigma[t], a.tmap[t], a.prec_unet[t] = float(tables["sigma"][t]), int(tables["tmap"][t]), prec
        a.prior_scale, a.scale_factor, a.prec_encode, a.prec_decode = float(tables["prior_scale"]), float(d.scale_factor), prec, prec
        rc = lib.rs_sample(h, C.byref(a))
    fam = (C.c_double * 96)()
    nf = lib.rs_profile_families(h, fam, 96)
    prof = (C.c_double * 9)()
    lib.rs_profile_get(h, prof)
    print(arg, "rc", rc, "err", repr(_lib.last_error()), "launches", lib.rs_last_launch_count(h),
          "families", ",".join(str(int(fam[3 * k + 2])) for k in range(nf)), "igemm", int(prof[3]), "gn", int(prof[7]), flush=True)


for arg in sys.argv[1:]:
    sys.stderr.write(f"case {arg}\n")
    sys.stderr.flush()
    run(arg)
