"""Static comparison of the stage kernels of two source trees: per kernel the register, scratch, spill, LDS and occupancy figures
hipcc reports (-Rpass-analysis=kernel-resource-usage, with build.py's flags) and whether the device assembly is the same.
Needs hipcc only, no GPU.  Prints one markdown table and the kernels whose occupancy, scratch, spills or LDS differ.

    python tools/kernel_resource_diff.py <parent tree> <refactored tree> [work dir]

`identical`: the instruction streams are equal once symbol names and the numbering of local labels are removed; `reordered`:
the same instructions in another order or with other register numbers; `differs`: anything else.  Kernels are matched by name;
RENAMED maps a parent kernel to the kernel(s) that took over its role."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from partsbaseddetector_amd import build  # noqa: E402

FILES = ["cloud", "planes", "consistency", "depth", "post", "publish", "qp", "features", "dp", "examples", "conv_mfma",
         "conv_mfma_any", "conv_mfma_f64"]
KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]"]
RENAMED = {
    "k_cl_scan_part<long long>": ["k_scan_part<long long, long long>"], "k_cl_scan_part<int>": ["k_scan_part<int, long long>"],
    "k_cl_scan_add<long long>": ["k_scan_add<long long, long long>"], "k_cl_scan_add<int>": ["k_scan_add<int, long long>"],
    "k_cl_scan_top": ["k_scan_top<long long, ClCropTotal>", "k_scan_top<long long, ScanNoTop>"],
    "k_pl_scan_part": ["k_scan_part<int, int>"], "k_pl_scan_top": ["k_scan_top<int, ScanNoTop>"],
    "k_pl_scan_add": ["k_scan_add<int, int>"],
    "k_resize": ["k_resize<unsigned char, Frames>"], "k_resize_runs": ["k_resize<unsigned char, Runs>"],
    "k_pyrdown": ["k_pyrdown<unsigned char, Frames>"], "k_pyrdown_runs<unsigned char, int, true>": ["k_pyrdown<unsigned char, Runs>"],
    "k_hog_grad<float>": ["k_hog_grad<float, unsigned char>"], "k_hog_grad<double>": ["k_hog_grad<double, unsigned char>"],
}
for _pt, _rw, _pw in (("unsigned short", "float", "int"), ("float", "float", "float"), ("double", "double", "double")):
    RENAMED["k_resize_t<%s, %s>" % (_pt, _rw)] = ["k_resize<%s, Frames>" % _pt]
    RENAMED["k_resize_runs_t<%s, %s>" % (_pt, _rw)] = ["k_resize<%s, Runs>" % _pt]
    RENAMED["k_pyrdown_t<%s, %s>" % (_pt, _pw)] = ["k_pyrdown<%s, Frames>" % _pt]
    RENAMED["k_pyrdown_runs<%s, %s, %s>" % (_pt, _pw, "true" if _pw == "int" else "false")] = ["k_pyrdown<%s, Runs>" % _pt]
    for _r in ("float", "double"):
        RENAMED["k_hog_grad_t<%s, %s>" % (_r, _pt)] = ["k_hog_grad<%s, %s>" % (_r, _pt)]

_tf = ("false", "true")
for _pt in ("unsigned char", "short"):
    for _bz in _tf:
        for _nw in _tf:
            for _r, _rh in (("float", "false"), ("float", "true"), ("double", "false")):      # the two passes are one kernel
                RENAMED["k_dt_rows<%s, %s, %s, %s, %s>" % (_r, _rh, _pt, _bz, _nw)] = ["k_dt_pass<%s, %s, %s, %s, %s, false>" % (_r, _rh, _pt, _bz, _nw)]
            for _r in ("float", "double"):
                RENAMED["k_dt_cols<%s, %s, %s, %s>" % (_r, _pt, _bz, _nw)] = ["k_dt_pass<%s, false, %s, %s, %s, true>" % (_r, _pt, _bz, _nw)]
    for _m in (2, 4, 6, 8, 16):                 # the combine kernels no longer carry the position planes' type
        for _r, _c, _rh in (("float", 4, "false"), ("float", 4, "true"), ("double", 2, "false")):
            RENAMED["k_dp_combine<%s, %d, %d, %s, %s>" % (_r, _c, _m, _rh, _pt)] = ["k_dp_combine<%s, %d, %d, %s>" % (_r, _c, _m, _rh)]
    for _r in ("float", "double"):
        RENAMED["k_dp_combine_seq<%s, %s>" % (_r, _pt)] = ["k_dp_combine_seq<%s>" % _r]


def compile_tree(tree, out):
    procs = []
    for f in FILES:
        src = os.path.join(tree, "partsbaseddetector_amd", "csrc", "pbd_kernels_%s.hip" % f)
        cmd = [build.hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o",
                                               os.path.join(out, f + ".s"), src]
        procs.append((f, subprocess.Popen(cmd, stderr=open(os.path.join(out, f + ".remarks"), "w"))))
    for f, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s of %s" % (f, tree))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d.replace("pbd::(anonymous namespace)::", "").replace("pbd::", ""))
        short[n] = re.sub(r"\((?!anonymous).*$", "", d)        # drop the parameter list, keep template arguments
    return short


def remarks(path):
    res, cur = collections.OrderedDict(), None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur:
            res[cur][m.group(1).strip()] = m.group(2)
    return res


def bodies(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or re.match(r"^\.Lfunc_end", line):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith("."):
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", s)))
    return out


def verdict(a, b):
    if a == b:
        return "identical"
    strip = lambda l: sorted(re.sub(r"\b[sv]\d+\b|\b[sv]\[\d+:\d+\]", "R", x) for x in l)   # noqa: E731
    return "reordered" if strip(a) == strip(b) else "differs"


def main():
    parent, new = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp()
    dirs = {}
    for tag, tree in (("parent", parent), ("refactored", new)):
        dirs[tag] = os.path.join(work, tag)
        os.makedirs(dirs[tag], exist_ok=True)
        compile_tree(tree, dirs[tag])
    print("| file | kernel (parent) | kernel (refactored) | SGPR | VGPR | AGPR | scratch | occupancy | spills S / V | LDS | instructions | assembly |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    bad, counts = [], collections.Counter()
    for f in FILES:
        rb, rn = remarks(os.path.join(dirs["parent"], f + ".remarks")), remarks(os.path.join(dirs["refactored"], f + ".remarks"))
        bb, bn = bodies(os.path.join(dirs["parent"], f + ".s")), bodies(os.path.join(dirs["refactored"], f + ".s"))
        names = demangle(list(rb) + list(rn))
        by_name = {names[k]: k for k in rn}
        for kb in rb:
            for target in RENAMED.get(names[kb], [names[kb]]) if names[kb] not in by_name else [names[kb]]:
                if target not in by_name:
                    print("| %s | `%s` | NOT FOUND: `%s` |" % (f, names[kb], target))
                    bad.append((f, names[kb], "missing"))
                    continue
                kn = by_name[target]
                x, y = rb[kb], rn[kn]
                c = lambda k: x[k] if x[k] == y[k] else "%s -> %s" % (x[k], y[k])   # noqa: E731
                la, lb = len(bb[kb]), len(bn[kn])
                v = verdict(bb[kb], bn[kn])
                counts[v] += 1
                print("| %s | `%s` | %s | %s | %s | %s | %s | %s | %s / %s | %s | %s | %s |" % (
                    f, names[kb], "same" if names[kb] == target else "`%s`" % target, c(KEYS[0]), c(KEYS[1]), c(KEYS[2]), c(KEYS[3]),
                    c(KEYS[4]), c(KEYS[5]), c(KEYS[6]), c(KEYS[7]), la if la == lb else "%d -> %d" % (la, lb), v))
                bad += [(f, names[kb], k, x[k], y[k]) for k in KEYS[3:] if x[k] != y[k]]
    print()
    print("assembly:", dict(counts))
    print("occupancy / scratch / spills / LDS differ:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
