"""Hash the gfx950 device code of every object of a build: one line per object with the sha256 (first 16 hex digits) of the
code object's .text and .rodata.  A change that touches host code only leaves every line as it was.

    python tools/device_code_hash.py [build directory, default loner_amd/_build] > table.txt
    python tools/device_code_hash.py --kernels <object file> > kernels.txt

--kernels: one line per function symbol of the object's code object (mangled name, size, sha256 of its bytes of .text), for a change
that removes kernels from an object.  A kernel that addresses .rodata PC-relatively changes its hash when code in front of it goes:
compare such a pair with llvm-objdump -d --no-show-raw-insn --disassemble-symbols=<name>.
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


def _code_object(tmp, obj):
    """The gfx950 code object of a host object, unbundled into tmp (None: no device code)."""
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    data = _section(tmp, obj, ".hip_fatbin")
    if data is None:
        return None
    open(fatbin, "wb").write(data)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fatbin}", f"--output={co}"], check=True, capture_output=True)
    return co


def device_hashes(obj):
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(tmp, obj)
        if co is None:
            return None
        return {s: (lambda d: hashlib.sha256(d).hexdigest()[:16] if d is not None else "-")(_section(tmp, co, s)) for s in (".text", ".rodata")}


def kernel_hashes(obj):
    """[(symbol, size, hash)] of every function of the object's code object, in address order."""
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(tmp, obj)
        if co is None:
            return []
        readelf = lambda *a: subprocess.run([os.path.join(LLVM, "llvm-readelf"), *a, "--wide", co], check=True, capture_output=True, text=True).stdout
        text_addr = next(int(f[f.index(".text") + 2], 16) for f in (l.replace("[", " ").replace("]", " ").split() for l in readelf("-S").splitlines()) if ".text" in f)
        text = _section(tmp, co, ".text")
        funcs = {}
        for f in (l.split() for l in readelf("--symbols").splitlines()):
            if len(f) == 8 and f[3] == "FUNC":
                funcs[f[7]] = (int(f[1], 16), int(f[2]))
        return [(n, size, hashlib.sha256(text[a - text_addr:a - text_addr + size]).hexdigest()[:16]) for n, (a, size) in sorted(funcs.items(), key=lambda kv: kv[1])]


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        for n, size, h in kernel_hashes(sys.argv[2]):
            print(f"{size:7d}  {h}  {n}")
        sys.exit(0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "loner_amd", "_build")
    for name in sorted(f for f in os.listdir(build) if f.endswith(".o")):
        h = device_hashes(os.path.join(build, name))
        print(f"{name:32s} .text {h['.text']}  .rodata {h['.rodata']}" if h else f"{name:32s} no device code")
