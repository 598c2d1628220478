"""Helper of tests/test_unet_blocks_cpu.py: one rs_unet_forward under RS_FAKE_DEVICE=1 (test-hooks library; every launch fails, the
bookkeeping of the dry and the real pass does not - see _fake_device_plumbing.py), untraced and then traced, at mixed per-image timesteps.
Prints the engine's "[fake device]" line of each call on stderr, one "CALL <untraced|traced> rc <rc> launches <n> records <n>" line per
call and one "REC <name> <B> <C> <H> <W>" line per debug-trace record of the traced call.
Usage: _fake_device_trace.py <config yaml name> <batch> <precision 0 fp16 | 1 fp32 | 2 split> [<latent h> <latent w>]
(the latent size defaults to the config's image_size; the lq / mask size follows from it by the config's lq_size / image_size ratio)"""
import ctypes as C
import os
import sys

os.environ["RS_FAKE_DEVICE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from resshift_amd import _lib  # noqa: E402
from resshift_amd.config import load_config, to_plain  # noqa: E402
from resshift_amd.engine import _fill_ae, _fill_unet  # noqa: E402

lib = _lib.load()
cname = sys.argv[1]
B = int(sys.argv[2])
prec = int(sys.argv[3])
up = to_plain(load_config(cname))["model"]["params"]
cfg = _lib.Config()
_fill_unet(cfg.unet, up)
cfg.has_unet = 1
cfg.enable_f16 = cfg.enable_f32 = cfg.enable_split = 1
h = lib.rs_create(C.byref(cfg))
assert h
lib.rs_bind_weight_blob(h, 256 * 1024, lib.rs_weight_bytes(h))   # fake, aligned address: never dereferenced on the host
assert lib.rs_weights_ready(h) == 0
hz, hl = int(up["image_size"]), int(up["lq_size"])
zh, zw = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (hz, hz)
lh, lw = zh * hl // hz, zw * hl // hz
ts = (C.c_int * B)(*[(7 * b) % 15 for b in range(B)])
mask = 4096 if up.get("cond_mask") else None
for name in ("untraced", "traced"):
    lib.rs_debug_enable(h, int(name == "traced"))
    rc = lib.rs_unet_forward(h, 4096, ts, 4096, mask, 4096, B, zh, zw, lh, lw, prec, None)
    sys.stderr.flush()
    print(f"CALL {name} rc {rc} launches {lib.rs_last_launch_count(h)} records {lib.rs_debug_count(h)}", flush=True)
buf = C.create_string_buffer(128)
dims = (C.c_int * 4)()
for i in range(lib.rs_debug_count(h)):
    assert lib.rs_debug_info(h, i, buf, 128, dims) == 0
    print("REC", buf.value.decode(), *dims, flush=True)
lib.rs_debug_enable(h, 0)
