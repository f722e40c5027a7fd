"""Per kernel of a `-S --cuda-device-only` listing: the register and scratch figures of its metadata entry and the waves per SIMD they
allow (make -C columbiaimagesearch_amd/csrc report-regs).  Reads the amdhsa.kernels metadata only, no instruction.  On gfx950 a SIMD
has 512 VGPRs per lane (architectural + accumulation, handed out in blocks of 8) and holds at most 8 waves; LDS and the workgroup size
can lower the figure further and are not looked at here.
usage: kernel_regs.py [--no-scratch SUBSTRING ...] build/x.s ...
--no-scratch: exit with status 1 when a kernel whose demangled name contains SUBSTRING has a private segment (spills to memory or a
run-time indexed array), or when no kernel has that name."""
import re, subprocess, sys

KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]
        return [re.sub(r"^void ", "", re.sub(r"\(.*", "", n)) for n in out]  # template arguments tell the instantiations apart
    except (OSError, subprocess.CalledProcessError):
        return names


def report(path):
    lines = open(path).read().split("\n")
    meta = "\n".join(lines[lines.index("amdhsa.kernels:"):]) if "amdhsa.kernels:" in lines else ""
    rows = []
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:  # kernel-level keys sit at an indent of four
        entry = "    " + entry
        get = lambda k: re.search(r"^    \.%s:\s+(\S+)" % k, entry, flags=re.M).group(1)
        rows.append([get("name")] + [int(get(k)) for k in KEYS])
    short = demangle([r[0] for r in rows])
    print("%s: %d kernels\n%6s %6s %6s %8s %6s  kernel" % (path, len(rows), "vgpr", "vspill", "sspill", "scratch", "waves"))
    for r, name in sorted(zip(rows, short), key=lambda t: t[1]):
        waves = min(8, 512 // max(8, (r[1] + 7) // 8 * 8))
        print("%6d %6d %6d %8d %6d  %s" % (r[1], r[2], r[3], r[4], waves, name[:120]))
    return {name: r[4] for r, name in zip(rows, short)}


if __name__ == "__main__":
    args, gated = sys.argv[1:], []
    while args and args[0] == "--no-scratch":
        gated.append(args[1])
        args = args[2:]
    scratch = {}
    for path in args:
        scratch.update(report(path))
    status = 0
    for want in gated:
        hit = {n: b for n, b in scratch.items() if want in n}
        if not hit:
            print("kernel_regs: no kernel named %s" % want)
            status = 1
        for n, b in sorted(hit.items()):
            if b:
                print("kernel_regs: %s has a private segment of %d bytes, 0 wanted" % (n, b))
                status = 1
    sys.exit(status)
