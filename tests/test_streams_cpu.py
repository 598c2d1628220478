"""The stream contract of include/resshift_hip.h ("work is enqueued on the caller's hipStream_t") as a text scan of the HIP sources: no
kernel launch names the null stream, and the calls that are ordered against the null stream or the whole device - hipMemset, hipMemcpy,
hipDeviceSynchronize - stay where they are today, each with its reason.  tests/test_streams_gpu.py runs the entry points on a side stream;
this scan keeps a new launch or copy from leaving the caller's stream where no GPU test happens to look."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resshift_amd", "csrc")

# (file, function) -> why a null-stream / device-wide call is right there.  Anything else fails with its file and line.
ALLOWED = {
    ("engine.hip", "rs_pack_weights"): "uploads the packed blob from host staging that is freed on return; no stream argument, once per process",
    ("engine.hip", "rs_weights_ready"): "reads the blob header and the per-layer flags back to the host; no stream argument - rs_bcast_weights "
                                        "synchronises its stream before it returns, so the bytes are there",
    ("engine.hip", "rs_debug_enable"): "frees the trace's capture region: copies of the last traced call may be in flight on any stream",
    ("ops.hip", "dev_copy"): "op-level test entries upload host weights; complete on return, and the entry frees them behind a stream sync",
    ("ops.hip", "frag_major_from_device_rows"): "op-level test entry repacks a caller's device operand on the host: waits for the caller's stream first",
    ("ops.hip", "rs_op_conv3x3_wino"): "RS_WINO_STAMPS (phase-timing builds): reads the stamps back after hipStreamSynchronize(st)",
    ("igemm2.hip", "rs_igemm2_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
    ("igemm_split.hip", "rs_igemm_split_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
    ("swin_mlp.hip", "rs_mlp_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
    ("win_attn_split.hip", "rs_attn_split_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
    ("igemm4_kernel.h", "rs_igemm4_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
    ("norm_attn.hip", "rs_attn_phase_cycles"): "RS_SPLIT_ABLATE builds only: stamp reader, no stream argument",
}
ORDERED_CALLS = ("hipMemset(", "hipMemcpy(", "hipDeviceSynchronize(")
NULL_STREAMS = {"0", "nullptr", "NULL", "hipStreamDefault", "hipStreamLegacy", "hipStreamPerThread"}

_FUNC = re.compile(r"^( {4})?(?!(?:if|for|while|switch|else|return|do|case)\b)[A-Za-z_][^=;(]*?\b([A-Za-z_]\w*)\s*\([^;]*$")


def strip_comments(text):
    """the source with comments blanked out, line structure kept"""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def enclosing_function(lines, i):
    """name of the function whose body holds line i: the nearest line above that opens a free function (column 0) or a member function
    (four spaces, ending in '{')"""
    for j in range(i, -1, -1):
        m = _FUNC.match(lines[j].rstrip())
        if m and (m.group(1) is None or lines[j].rstrip().endswith("{")):
            return m.group(2)
    return "<file scope>"


def ordered_calls(name, text):
    """[(function, line number, call)] of every hipMemset( / hipMemcpy( / hipDeviceSynchronize( of a source"""
    lines = strip_comments(text).split("\n")
    out = []
    for i, line in enumerate(lines):
        for call in ORDERED_CALLS:
            for m in re.finditer(r"(?<![A-Za-z0-9_])" + re.escape(call), line):
                out.append((enclosing_function(lines, i), i + 1, call))
    return out


def launch_streams(text):
    """[(line number, stream argument)] of every hipLaunchKernelGGL of a source: the fifth argument, casts removed"""
    text = strip_comments(text)
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\s*\(", text):
        depth, args, cur, k = 1, [], "", m.end()
        while depth:
            c = text[k]
            depth += c in "([{"
            depth -= c in ")]}"
            if c == "," and depth == 1:
                args.append(cur)
                cur = ""
            elif depth:
                cur += c
            k += 1
        args.append(cur)
        stream = re.sub(r"\(\s*hipStream_t\s*\)", "", args[4]).replace("\\", "").strip() if len(args) > 4 else "<missing>"
        while stream.startswith("(") and stream.endswith(")"):
            stream = stream[1:-1].strip()
        out.append((text.count("\n", 0, m.start()) + 1, stream))
    return out


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 30, files
    for f in files:
        with open(f) as fh:
            yield os.path.basename(f), fh.read()


def violations(named_sources):
    bad = []
    for name, text in named_sources:
        for line, stream in launch_streams(text):
            if stream in NULL_STREAMS or stream == "<missing>":
                bad.append(f"{name}:{line}: hipLaunchKernelGGL on the null stream ({stream})")
        for i, line in enumerate(strip_comments(text).split("\n")):
            if "<<<" in line:
                bad.append(f"{name}:{i + 1}: a <<< >>> launch (use hipLaunchKernelGGL with the caller's stream)")
        for fn, line, call in ordered_calls(name, text):
            if (name, fn) not in ALLOWED:
                bad.append(f"{name}:{line}: {call[:-1]} in {fn}() - not on the caller's stream, and not on the allow-list")
    return bad


def test_no_launch_or_copy_leaves_the_callers_stream():
    bad = violations(sources())
    assert not bad, "\n".join(bad)


def test_every_allowed_site_still_exists():
    """an entry whose call is gone is removed from the list, so that the list stays what the sources do"""
    seen = {(name, fn) for name, text in sources() for fn, _, _ in ordered_calls(name, text)}
    assert seen == set(ALLOWED), (sorted(set(ALLOWED) - seen), sorted(seen - set(ALLOWED)))


def test_the_scan_sees_every_launch():
    n = sum(len(launch_streams(text)) for _, text in sources())
    raw = sum(len(re.findall(r"hipLaunchKernelGGL\s*\(", strip_comments(text))) for _, text in sources())
    assert n == raw and n > 100, (n, raw)


@pytest.mark.parametrize("paste, what", [
    ("    (void)hipMemset(out, 0, 16);\n", "hipMemset in"),
    ("    (void)hipMemcpy(out, in, 16, hipMemcpyDeviceToDevice);\n", "hipMemcpy in"),
    ("    (void)hipDeviceSynchronize();\n", "hipDeviceSynchronize in"),
    ("    hipLaunchKernelGGL((some_kernel<float, 4>), dim3(1), dim3(64), 0, 0, out);\n", "null stream (0)"),
    ("    hipLaunchKernelGGL(some_kernel, dim3(a > 1 ? a : b, 1), dim3(64), 0,\n        (hipStream_t)nullptr, out);\n", "null stream (nullptr)"),
    ("    some_kernel<<<dim3(1), dim3(64), 0, st>>>(out);\n", "<<< >>>"),
])
def test_a_pasted_null_stream_call_is_found(paste, what):
    """the scan on a scratch copy of resize.hip with the line pasted into rs_resize's body"""
    with open(os.path.join(CSRC, "resize.hip")) as fh:
        text = fh.read()
    assert not violations([("resize.hip", text)])
    at = text.index("{", text.index("int rs_resize(")) + 2
    bad = violations([("resize.hip", text[:at] + paste + text[at:])])
    assert len(bad) == 1 and what in bad[0] and bad[0].startswith("resize.hip:"), bad
    if "in" == what.split()[-1]:
        assert "rs_resize()" in bad[0], bad
