"""Register / LDS / scratch table of the built kernels: unbundles the gfx950 code objects from rlaif-v_amd/build/*.o and reads
their metadata notes.  Usage: python tools/kernel_resources.py [substring] [--build DIR]
--digest: per object, every device function's mangled name, size and SHA-256 of its bytes in .text, sorted by name.  Equal
listings mean equal device code.  Whole objects differ with the order in which the host code instantiates the kernels; a
function's own bytes do not - UNLESS it addresses a device global relative to the program counter, as the four
gemm_tn_256_kernel instantiations do with g_zero_row: their digests change when the layout of .text does (another
instantiation order, a kernel before them that grew), with not one instruction different.  Read a difference in those four
alone as "moved" and compare their disassembly before calling it a code change."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _objects(build_dir):
    return [o for o in sorted(os.listdir(build_dir)) if o.endswith(".o")]


def _unbundle(obj, td):
    """the gfx950 code object of a host object file"""
    fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fat}", f"--output={co}", "--unbundle"], check=True)
    return co


def digests(build_dir):
    """[(object, mangled name, size, sha256 of the function's bytes)], sorted by object and name"""
    out = set()                                   # (.dynsym and .symtab list the same functions)
    for o in _objects(build_dir):
        with tempfile.TemporaryDirectory() as td:
            co = _unbundle(os.path.join(build_dir, o), td)
            elf = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
            blob = open(co, "rb").read()
        m = re.search(r"\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", elf)
        ndx, addr, off = m.group(1), int(m.group(2), 16), int(m.group(3), 16)
        for line in elf.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC" and f[6] == ndx:
                start, size = off + int(f[1], 16) - addr, int(f[2])
                out.add((o, f[7], size, hashlib.sha256(blob[start:start + size]).hexdigest()))
    return sorted(out)


def resources(build_dir):
    rows = []
    for o in _objects(build_dir):
        with tempfile.TemporaryDirectory() as td:
            co = _unbundle(os.path.join(build_dir, o), td)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            dem = {}
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"\s+-?\s*\.(\w+):\s+(.*)", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip().strip("'")
                if k == "agpr_count" and cur.get("name"):
                    pass
                if k in ("agpr_count",) and "agpr_count" in cur:
                    rows.append(cur)
                    cur = {}
                cur[k] = v
                if k == "wavefront_size":
                    rows.append(cur)
                    cur = {}
    out = []
    for r in rows:
        if "name" not in r:
            continue
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::|void ", "", name).split("(")[0]
        out.append((name, int(r.get("vgpr_count", 0)), int(r.get("agpr_count", 0)), int(r.get("sgpr_count", 0)),
                    int(r.get("vgpr_spill_count", 0)), int(r.get("group_segment_fixed_size", 0)),
                    int(r.get("private_segment_fixed_size", 0))))
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bd = "build"
    if "--build" in sys.argv:
        bd = sys.argv[sys.argv.index("--build") + 1]
        args = [a for a in args if a != bd]
    sub = args[0] if args else ""
    if "--digest" in sys.argv:
        for o, name, size, sha in digests(os.path.join(REPO, "rlaif-v_amd", bd)):
            if sub in name:
                print(f"{o} {name} {size} {sha}")
        sys.exit(0)
    print(f"{'kernel':100s} {'vgpr':>5s} {'agpr':>5s} {'sgpr':>5s} {'spill':>5s} {'lds':>7s} {'scratch':>7s}")
    for r in resources(os.path.join(REPO, "rlaif-v_amd", bd)):
        if sub in r[0]:
            print(f"{r[0][:100]:100s} {r[1]:5d} {r[2]:5d} {r[3]:5d} {r[4]:5d} {r[5]:7d} {r[6]:7d}")
