"""Digest of the device code of every kernel, per source file: the check of a refactor that must leave the kernels alone.

    python tools/device_code_digest.py [--against <other checkout>]

Every file of build.SOURCES is compiled with build.FLAGS + --cuda-device-only -S (no GPU needed) and the assembly is cut per
.amdhsa_kernel symbol: the function's text from its label to its .size line, plus its .amdhsa_* block (registers, scratch, LDS).
Printed per file: the kernel count and the sha256 of the per-kernel texts sorted by symbol.  With --against, the same for the
other checkout's sources (compiled with THIS checkout's flags), and whether the symbol sets, every kernel's text and the order
of the kernels are equal; the kernels that differ are named and the exit status is 1.  A file of build.SOURCES that the other
checkout does not have is listed with its own count and digest and compared with nothing.  With --renamed as well, a file that
differs is compared once more kernel by kernel after renaming: the symbol itself, a trailing default template argument a kernel
template gained (`Li0E`, and with it an argument type that depends on it), the function number in local labels (.LBB<n>_, .Lfunc_end<n>) and the assembly comments (which name
blocks by function number) are taken out, and the other checkout's kernels are listed as `same` / `DIFF` with the new symbols and
whether the old ones kept their order."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from faceformer_amd.hip import build  # noqa: E402


def kernels(root, src, tmp):
    """[(symbol, text)] of one source file of the checkout at `root`, in the order of the assembly."""
    out = os.path.join(tmp, "%s.%s.s" % (hashlib.sha256(root.encode()).hexdigest()[:8], src))
    flags = [f for f in build.FLAGS if not f.startswith("-I")]
    flags += ["-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "faceformer_amd", "csrc")]
    subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out,
                    os.path.join(root, "faceformer_amd", "csrc", src)], check=True, stderr=subprocess.DEVNULL)
    s = open(out).read()
    res = []
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel\n", s, re.M | re.S):
        sym = m.group(1)
        a = s.index("\n%s:" % sym) + 1
        b = re.compile(r"^\s*\.size\s+%s,.*\n" % re.escape(sym), re.M).search(s, a).end()
        res.append((sym, s[a:b] + m.group(0)))
    return res


def renamed(ks):
    """{symbol without an added default template argument: text with symbol, label numbers and comments taken out}, order."""
    out, order = {}, []
    for sym, t in ks:
        name = re.sub(r"ELi0EEEvT_$", "EEEvT_", sym)
        # (a kernel whose argument struct now depends on the added argument: `<W, STOP, FORM = 0>(SeqConBeamArgsOf<FORM>::type)`)
        name = re.sub(r"ELi0EEEvNS_16SeqConBeamArgsOfIXT1_EE4typeE$", "EEEvNS_14SeqConBeamArgsE", name)
        t = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1n", t.replace(sym, "SYM"))
        out[name] = "\n".join(re.sub(r"\s*;.*$", "", line).rstrip() for line in t.splitlines())
        order.append(name)
    return out, order


def digest(ks):   # (symbol, newline, text -- the form whose digests profiles/launch_layer/device_code.txt recorded)
    return hashlib.sha256("".join(k + "\n" + t for k, t in sorted(ks)).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--against", metavar="CHECKOUT", help="compare with the sources of another checkout of this repository")
    ap.add_argument("--renamed", action="store_true", help="with --against: compare a differing file again after renaming")
    args = ap.parse_args()
    roots = [ROOT] + ([os.path.abspath(args.against)] if args.against else [])
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        jobs = {(r, src): pool.submit(kernels, r, src, tmp) for r in roots for src in build.SOURCES
                if os.path.exists(os.path.join(r, "faceformer_amd", "csrc", src))}      # (a file only this checkout has: see below)
        got = {k: f.result() for k, f in jobs.items()}
    print("flags: " + " ".join(build.FLAGS).replace(ROOT + os.sep, "") + " --cuda-device-only -S")
    bad = 0
    for src in build.SOURCES:
        new = got[(ROOT, src)]
        if not args.against:
            print("%s: %d kernels  sha256 %s" % (src, len(new), digest(new)))
            continue
        if (roots[1], src) not in got:
            print("%s: not in the other checkout, %d kernels here  sha256 %s" % (src, len(new), digest(new)))
            continue
        old = got[(roots[1], src)]
        dn, do = dict(new), dict(old)
        differ = sorted(set(dn) ^ set(do)) + sorted(k for k in set(dn) & set(do) if dn[k] != do[k])
        same_order = [k for k, _ in new] == [k for k, _ in old]
        ok = not differ and same_order
        bad += not ok
        print("%s: %d kernels other, %d here: %s" % (src, len(old), len(new), "identical, same order" if ok else "DIFFERENT"))
        print("  symbol sets %s, kernel order %s" % ("equal" if set(dn) == set(do) else "DIFFER", "equal" if same_order else "DIFFERS"))
        print("  sha256 other %s\n  sha256 here  %s" % (digest(old), digest(new)))
        for k in differ:
            print("  differs: " + k)
        if args.renamed and not ok:
            (rn, on), (ro, oo) = renamed(new), renamed(old)
            for k in oo:
                print("  after renaming: %s  %s" % ("same" if rn.get(k) == ro[k] else "DIFF", k))
            print("  after renaming: %d new symbols; the other checkout's kernels keep their order: %s"
                  % (len([k for k in on if k not in ro]), [k for k in on if k in ro] == oo))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
