"""name, code size and SHA-256 of the code bytes of every gfx950 kernel of a built library (each kernel symbol's range in .text, read with
llvm-readelf -S -s; no GPU needed).  With two libraries: every kernel of the second whose bytes match no kernel of the first - by bytes,
not by name, because names change with the template arguments.
    python scripts/kernel_digest.py LIB.so [NEW.so]"""
import hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from resshift_amd.build import gfx950_code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def digests(lib_path):
    """{kernel name: (code bytes, sha256)} - a kernel is a FUNC symbol that has a kernel descriptor (NAME.kd)"""
    out = {}
    for co in gfx950_code_objects(lib_path):
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(co)
            fh.flush()
            txt = subprocess.run([READELF, "-S", "-s", "-W", fh.name], capture_output=True, text=True, check=True).stdout
        nr, addr, off = re.search(r"\[\s*(\d+)\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+)", txt).groups()
        syms = re.findall(r"^\s*\d+: ([0-9a-f]+)\s+(\d+) (FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+) (\S+)$", txt, re.M)
        kd = {name[:-3] for _, _, typ, _, name in syms if typ == "OBJECT" and name.endswith(".kd")}
        for val, size, typ, ndx, name in syms:
            if typ == "FUNC" and ndx == nr and name in kd:
                start = int(val, 16) - int(addr, 16) + int(off, 16)
                out[name] = (int(size), hashlib.sha256(co[start:start + int(size)]).hexdigest())
    return out


if __name__ == "__main__":
    base = digests(sys.argv[1])
    if len(sys.argv) == 2:
        for name, (size, sha) in sorted(base.items()):
            print(f"{sha} {size:7d} {name}")
    else:
        new, seen = digests(sys.argv[2]), {v for v in base.values()}
        odd = sorted(name for name, v in new.items() if v not in seen)
        for name in odd:
            print(f"no match in {sys.argv[1]}: {new[name][0]:7d} bytes {name}")
        print(f"{sys.argv[1]}: {len(base)} kernels, {os.path.getsize(sys.argv[1])} bytes")
        print(f"{sys.argv[2]}: {len(new)} kernels, {os.path.getsize(sys.argv[2])} bytes; {len(new) - len(odd)} byte-identical to a kernel of the first, {len(odd)} not")
        sys.exit(1 if odd else 0)
