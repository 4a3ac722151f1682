"""One line per kernel of the given HIP sources: registers, scratch, LDS, occupancy, instruction counts by class and a SHA-1 of
the instruction stream -- so that two versions of a source can be compared kernel by kernel without a GPU.

    python tools/kernel_table.py [--csrc DIR] [--flags "..."] linear.hip token_h2.hip ...      (names relative to DIR)

Each source is compiled with the product flags of objcavit_amd/build.py plus ``--cuda-device-only -S`` (about 4 s per file).
Columns: VGPRs AGPRs SGPRs scratch[B/lane] static-LDS[B] occupancy[waves/SIMD] (the assembly's kernel metadata) | instructions,
matrix instructions, LDS reads, LDS writes, vector-memory loads, vector-memory stores, s_barrier, s_waitcnt | SHA-1 of the
instruction stream with labels, comments and directives stripped (branch targets keep their number within the function, not the
function's index in its file, so a kernel that moves to another file keeps its SHA; a symbol addressed pc-relative -- a zero page,
say -- counts as SYM, so renaming it is not another stream).

    python tools/kernel_table.py --compare PARENT.txt NEW.txt       compares two saved tables by kernel name
    python tools/kernel_table.py --stream KERNEL SOURCE.hip         the stripped stream of one kernel, to diff two versions of it
"""
import argparse, hashlib, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast"]        # objcavit_amd/build.py
CLASSES = (("mfma", re.compile(r"^v_s?mfma")), ("lds_rd", re.compile(r"^ds_(read|load)")), ("lds_wr", re.compile(r"^ds_(write|store)")),
           ("vm_ld", re.compile(r"^(global|buffer|flat|scratch)_load")), ("vm_st", re.compile(r"^(global|buffer|flat|scratch)_store")),
           ("barrier", re.compile(r"^s_barrier")), ("waitcnt", re.compile(r"^s_waitcnt")))
COLS = "VGPR AGPR SGPR scratch LDS occ | insts mfma lds_rd lds_wr vm_ld vm_st barrier waitcnt | stream-sha1"


def _tool(*names):
    for name in names:
        for c in (shutil.which(name), "/opt/rocm/llvm/bin/" + name, "/opt/rocm/bin/" + name):
            if c and os.path.exists(c):
                return c
    raise RuntimeError(" / ".join(names) + " not found")


def assembly(path, extra):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run([_tool("hipcc")] + FLAGS + extra + ["--cuda-device-only", "-S", path, "-o", out], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {path}:\n{r.stdout}")
        return open(out).read()


def kernels(asm):
    """{mangled name: row dict} of every kernel in one assembly file"""
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm.split("amdhsa.kernels:")[1])[1:]:
        f = dict(re.findall(r"^(?:    |  - )\.(\w+):\s+(\S+)", "  - .agpr_count:" + blk.split("\namdhsa.")[0], re.M))   # kernel-level keys only
        meta[f["name"]] = f
    rows = {}
    for name, f in meta.items():
        body = asm.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        occ = re.search(r"; Occupancy: (\d+)", asm.split("\n" + name + ":", 1)[1])
        stream = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            stream.append(re.sub(r"[\w$.]+@(gotpcrel32|rel32)", r"SYM@\1", re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", line))))
        row = {"vgpr": int(f["vgpr_count"]), "agpr": int(f["agpr_count"]), "sgpr": int(f["sgpr_count"]),
               "scratch": int(f["private_segment_fixed_size"]), "lds": int(f["group_segment_fixed_size"]),
               "occ": int(occ.group(1)) if occ else -1, "insts": len(stream)}
        for cls, rx in CLASSES:
            row[cls] = sum(1 for s in stream if rx.match(s))
        row["sha"] = hashlib.sha1("\n".join(stream).encode()).hexdigest()[:16]
        row["stream"] = stream
        rows[name] = row
    return rows


def demangle(names):
    r = subprocess.run([_tool("llvm-cxxfilt", "c++filt")], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
    out = []
    for n in r.stdout.splitlines():
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n)            # a mangling the demangler at hand does not know (_Float16 arguments): the bare name
        n = n[m.end():m.end() + int(m.group(1))] if m else n
        out.append(re.sub(r"^void \(anonymous namespace\)::|^\(anonymous namespace\)::|\(.*\)$", "", n.strip().removeprefix("void ")))
    return out


def fmt(r):
    return (f"{r['vgpr']} {r['agpr']} {r['sgpr']} {r['scratch']} {r['lds']} {r['occ']} | {r['insts']} " +
            " ".join(str(r[c]) for c, _ in CLASSES) + f" | {r['sha']}")


def table(csrc, sources, extra):
    lines = []
    for src in sources:
        rows = kernels(assembly(os.path.join(csrc, src), extra))
        names = list(rows)
        for n, d in sorted(zip(demangle(names), names)):
            lines.append(f"{src}: {n}: {fmt(rows[d])}")
    return lines


def compare(parent, new):
    def load(p):
        out = {}
        for line in open(p):
            m = re.match(r"\s*(\S+\.hip): (.*?): (\d.*\| \w+)\s*$", line)
            if m:
                out[m.group(2)] = (m.group(1), m.group(3))
        return out
    a, b = load(parent), load(new)
    nsha = nres = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}: {'NEW' if k not in a else 'GONE'} ({(a.get(k) or b.get(k))[0]})")
            continue
        (fa, ra), (fb, rb) = a[k], b[k]
        where = fa if fa == fb else f"{fa} -> {fb}"
        if ra == rb:
            print(f"{k} [{where}]: SAME  {rb}")
            continue
        ca, cb = ra.split(" | "), rb.split(" | ")
        res = [x for i, x in enumerate(ca[0].split()) if i >= 3] != [x for i, x in enumerate(cb[0].split()) if i >= 3]
        nsha += 1
        nres += res
        print(f"{k} [{where}]: STREAM DIFFERS{'  (scratch / LDS / occupancy differ)' if res else ''}\n      parent {ra}\n      new    {rb}")
    print(f"kernels: parent {len(a)}, new {len(b)}; stream differs: {nsha}; scratch / static LDS / occupancy differ: {nres}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "objcavit_amd", "csrc"))
    ap.add_argument("--flags", default="", help="extra compiler flags")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--stream", metavar="KERNEL", help="print the stripped instruction stream of the kernel with this demangled name (for diff)")
    ap.add_argument("sources", nargs="*")
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
    elif a.stream:
        for src in a.sources:
            rows = kernels(assembly(os.path.join(a.csrc, src), a.flags.split()))
            for n, d in zip(demangle(list(rows)), list(rows)):
                if n == a.stream:
                    print("\n".join(rows[d]["stream"]))
    else:
        print("# " + COLS)
        print("\n".join(table(a.csrc, a.sources, a.flags.split())))
