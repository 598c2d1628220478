"""Helper of tests/test_large_tensors_cpu.py, a sibling of _fake_device_structures.py for the shipped configs' autoencoders: with
RS_FAKE_DEVICE=1 the engine walks its control flow on a host-memory arena while every launch fails.  One process runs any number of cases,
one argument each:

    <config yaml name>:<encode | decode>:<batch>:<precision 0 fp16 | 1 fp32 | 2 split>

at the config's own resolution.  Per case, on stdout: "<argument> rc <rc> launches <n> err <rs_last_error>"."""
import ctypes as C
import os
import sys

os.environ["RS_FAKE_DEVICE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resshift_amd import _lib  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.engine import _fill_ae  # noqa: E402

lib = _lib.load()
FAKE = 4096   # a fake, aligned device address: never dereferenced on the host
_engines = {}


def engine(name):
    if name not in _engines:
        ap = to_plain(load_config(name))["autoencoder"]["params"]
        cfg = _lib.Config()
        _fill_ae(cfg.ae, ap)
        cfg.has_ae = 1
        cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
        h = lib.rs_create(C.byref(cfg))
        assert h, _lib.last_error()
        lib.rs_bind_weight_blob(h, 256 * 1024, lib.rs_weight_bytes(h))
        assert lib.rs_weights_ready(h) == 0
        _engines[name] = (h, ap)
    return _engines[name]


for arg in sys.argv[1:]:
    name, call, B, prec = arg.split(":")
    h, ap = engine(name)
    dd = ap["ddconfig"]
    res, f = int(dd["resolution"]), 2 ** (len(dd["ch_mult"]) - 1)
    sys.stderr.write(f"case {arg}\n")
    sys.stderr.flush()
    if call == "encode":
        rc = lib.rs_vq_encode(h, FAKE, FAKE, int(B), res, res, int(prec), None)
    else:
        rc = lib.rs_vq_decode(h, FAKE, FAKE, FAKE, int(B), res // f, res // f, 0, int(prec), None)
    print(arg, "rc", rc, "launches", lib.rs_last_launch_count(h), "err", _lib.last_error(), flush=True)
