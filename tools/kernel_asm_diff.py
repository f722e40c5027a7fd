"""Proof that a host-side change left the device code alone: every kernel of the `-S --cuda-device-only` listings before `--` against
the kernel of the same name in the listings after it (make -C columbiaimagesearch_amd/csrc build/x.s).  Compared per kernel: the
instruction text of the body, the .amdhsa_* descriptor and the register / spill / scratch / LDS figures of the metadata; only local
label numbers, line-info directives and comments are normalised.  Exit status 1 when a kernel is missing, new or different.
--removed SUBSTRING (may be repeated): a kernel of the old side only whose mangled or demangled name contains SUBSTRING was removed on
purpose: it is printed as `removed:` and is no failure.
usage: kernel_asm_diff.py old/lopq_search.s -- new/lopq_search.s new/lopq_plan.s [--removed k_old_kernel]"""
import difflib, re, shutil, subprocess, sys

META = r"^    \.(vgpr_spill_count|sgpr_spill_count|vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):"


def norm(line):
    line = line.split(";")[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.L(tmp|func_begin|func_end|BB_end|sec_end|post_getpc)\d+", r".L\1", line)


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        for i, l in enumerate(lines):
            m = re.match(r"^\s*\.amdhsa_kernel (\S+)", l)
            if m:  # the body runs from the kernel's label to its descriptor
                name = m.group(1)
                assert name not in out, "kernel defined twice: " + name
                body = [norm(t) for t in lines[next(j for j, t in enumerate(lines) if t.startswith(name + ":")) + 1:i] if not re.match(r"^\s*\.(loc|file|cfi_)", t)]
                desc = [norm(t) for t in lines[i + 1:lines.index("\t.end_amdhsa_kernel", i)]]
                out[name] = [t for t in body if t.strip()] + ["-- descriptor --"] + desc
        meta = "\n".join(lines[lines.index("amdhsa.kernels:"):]) if "amdhsa.kernels:" in lines else ""
        for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:  # kernel-level keys sit at an indent of four
            name = re.search(r"^    \.name:\s+(\S+)", entry, flags=re.M).group(1)
            out[name] += ["-- metadata --"] + [l for l in ("    " + entry).split("\n") if re.match(META, l)]
    return out


def demangled(name):  # "k<4, 2>" of "void k<4, 2>(int const*)"; the mangled name where there is no c++filt
    if not shutil.which("c++filt"):
        return name
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "")


args, removed = sys.argv[1:], []
while "--removed" in args:
    i = args.index("--removed")
    removed.append(args[i + 1])
    del args[i:i + 2]
sep = args.index("--")
old, new = kernels(args[:sep]), kernels(args[sep + 1:])
bad = 0
for name in sorted(set(old) | set(new)):
    if name not in new and any(r in name or r in demangled(name) for r in removed):
        print("removed: %s" % demangled(name))
    elif name not in old or name not in new:
        print("%s only: %s" % ("old" if name in old else "new", name))
        bad += 1
    elif old[name] != new[name]:
        print("DIFFERENT: %s" % name)
        print("\n".join(list(difflib.unified_diff(old[name], new[name], "old", "new", lineterm="", n=2))[:60]))
        bad += 1
print("%d kernels before, %d after, %d missing / new / different" % (len(old), len(new), bad))
sys.exit(1 if bad else 0)
