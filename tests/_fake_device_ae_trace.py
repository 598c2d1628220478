"""Helper of tests/test_ae_blocks_cpu.py: one rs_vq_encode or rs_vq_decode under RS_FAKE_DEVICE=1 (test-hooks library; every launch fails,
the bookkeeping of the dry and the real pass does not - see _fake_device_plumbing.py), untraced and then traced.
Prints the engine's "[fake device]" line of each call on stderr, one "CALL <untraced|traced> rc <rc> launches <n> records <n>" line per
call and one "REC <name> <B> <C> <H> <W>" line per debug-trace record of the traced call.
Usage: _fake_device_ae_trace.py <config yaml name> <encode|decode|decode_nq> <batch> <H> <W> <precision 0 fp16 | 1 fp32 | 2 split>
(H, W: the image for encode, the latent for decode)"""
import ctypes as C
import os
import sys

os.environ["RS_FAKE_DEVICE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from resshift_amd import _lib  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.engine import _fill_ae  # noqa: E402

lib = _lib.load()
cname, call = sys.argv[1], sys.argv[2]
B, Hh, Ww, prec = (int(v) for v in sys.argv[3:7])
ap = to_plain(load_config(cname))["autoencoder"]["params"]
cfg = _lib.Config()
_fill_ae(cfg.ae, ap)
cfg.has_ae = 1
cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
h = lib.rs_create(C.byref(cfg))
assert h
lib.rs_bind_weight_blob(h, 256 * 1024, lib.rs_weight_bytes(h))   # fake, aligned address: never dereferenced on the host
assert lib.rs_weights_ready(h) == 0
for name in ("untraced", "traced"):
    lib.rs_debug_enable(h, int(name == "traced"))
    if call == "encode":
        rc = lib.rs_vq_encode(h, 4096, 4096, B, Hh, Ww, prec, None)
    else:
        rc = lib.rs_vq_decode(h, 4096, 4096, 4096, B, Hh, Ww, int(call == "decode_nq"), prec, None)
    sys.stderr.flush()
    print(f"CALL {name} rc {rc} launches {lib.rs_last_launch_count(h)} records {lib.rs_debug_count(h)}", flush=True)
buf = C.create_string_buffer(128)
dims = (C.c_int * 4)()
for i in range(lib.rs_debug_count(h)):
    assert lib.rs_debug_info(h, i, buf, 128, dims) == 0
    print("REC", buf.value.decode(), *dims, flush=True)
lib.rs_debug_enable(h, 0)
