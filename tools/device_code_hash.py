"""Hash the gfx950 device code of every object of a build: one line per object with the sha256 (first 16 hex digits) of the
code object's .text and .rodata.  A change that touches host code only leaves every line as it was.

    python tools/device_code_hash.py [build directory, default loner_amd/_build] > table.txt
"""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def _section(tmp, src, name):
    out = os.path.join(tmp, "section")
    if os.path.exists(out):
        os.remove(out)
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section={name}={out}", src], capture_output=True)
    return open(out, "rb").read() if os.path.exists(out) else None


def device_hashes(obj):
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        data = _section(tmp, obj, ".hip_fatbin")
        if data is None:
            return None
        open(fatbin, "wb").write(data)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fatbin}", f"--output={co}"], check=True, capture_output=True)
        return {s: (lambda d: hashlib.sha256(d).hexdigest()[:16] if d is not None else "-")(_section(tmp, co, s)) for s in (".text", ".rodata")}


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "loner_amd", "_build")
    for name in sorted(f for f in os.listdir(build) if f.endswith(".o")):
        h = device_hashes(os.path.join(build, name))
        print(f"{name:32s} .text {h['.text']}  .rodata {h['.rodata']}" if h else f"{name:32s} no device code")
