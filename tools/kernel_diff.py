#!/usr/bin/env python3
"""Generated-code comparison of the device units (the stage units scan_columns / align / trace / mailbox / setup .hip, which replaced
kernels.hip, select / hits / binned .hip, and the guide-site units sites / near_list / activity / site_regions / site_pairs / allele_sites / microhomology / edit_sites .hip) against an earlier revision: the check that a move or a refactor of device code left the
compiler's output as it was.

  python tools/kernel_diff.py [--rev HEAD~1] [--show]

1. `git archive REV calitas_amd/csrc include` into a temporary directory; every .hip file of the list below that exists there (kernels.hip
   before the split) and every one of the working tree is compiled with
   `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S` (the flags of the Makefile).
2. Every function of the output (the kernels, and replay_word, which the compiler keeps out of line) is cut from its label to
   .Lfunc_end; comments, directives and the function's index in the labels (.LBB<k>_<n>) are dropped.  rocPRIM's own kernels (the
   sort and the scan hits.hip and select.hip instantiate: mangled names beginning _ZN7rocprim) are skipped.
3. Per kernel: identical or not; VGPRs, SGPRs, LDS bytes and scratch of both; the instruction count of every innermost loop that
   shifts values down the lanes (`wave_shr:1`: the fill loops of the aligners), and whether those loops differ in more than the
   numbers of their registers.  --show prints the unified diff of a kernel that
   differs.
A kernel the revision does not have is listed as new with its resources.
Exit status 1 when a kernel differs or one of the revision's is missing."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("calitas_amd", "csrc")
UNITS = ["kernels.hip", "scan_columns.hip", "align.hip", "trace.hip", "mailbox.hip", "setup.hip", "select.hip", "hits.hip", "binned.hip", "sites.hip",
         "near_list.hip", "activity.hip", "site_regions.hip", "site_pairs.hip", "allele_sites.hip", "microhomology.hip", "edit_sites.hip"]


def device_asm(csrc, out_dir):
    text = ""
    for u in UNITS:
        src = os.path.join(csrc, u)
        if not os.path.exists(src):
            continue
        out = os.path.join(out_dir, u + ".s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", out],
                              stderr=subprocess.DEVNULL)
        text += open(out).read()
    return text


def functions_of(asm):
    """name -> {code: normalised lines, raw: lines as they came, vgpr, sgpr, lds, scratch}"""
    out = {}
    lines = asm.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m or m.group(1).startswith("_ZN7rocprim"):     # (rocPRIM's: hundreds of kernels, and variables that end in no .Lfunc_end)
            i += 1
            continue
        name, raw = m.group(1), []
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            raw.append(lines[i])
            i += 1
        code = []
        for ln in raw:
            t = ln.split(";")[0].rstrip()
            if not t.strip() or (t.strip().startswith(".") and not re.match(r"^\.LBB\d+_\d+:", t)):
                continue
            if ".amdhsa_kernel" in t:
                break
            code.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
        f = {"code": code, "raw": raw}
        for j in range(i, min(i + 60, len(lines))):               # the "Kernel info" comment behind the function
            for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("scratch", r"; ScratchSize: (\d+)")):
                k = re.match(pat, lines[j])
                if k and key not in f:
                    f[key] = int(k.group(1))
            if re.match(r"^_Z\w+:", lines[j]):
                break
        out[name] = f
    return out


def lane_shift_loops(raw):
    """The innermost loops that hold a `wave_shr:1`, in layout order: [instruction count, text with the register numbers dropped]."""
    loops, order = {}, []
    header = None
    for k, ln in enumerate(raw):
        if re.match(r"^\.LBB\d+_\d+:", ln) or ln.startswith("; %bb."):
            note = " ".join([ln] + [x for x in raw[k + 1:k + 4] if x.strip().startswith(";") and "%bb." not in x])
            h = re.search(r"^\.L(BB\d+_\d+):.*This Inner Loop Header", note)
            g = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            header = h.group(1) if h else (g.group(1) if g and g.group(1) in loops else None)
            if h:
                loops[header] = [0, False, []]
                order.append(header)
            continue
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") or header is None:
            continue
        loops[header][0] += 1
        loops[header][1] = loops[header][1] or "wave_shr:1" in t
        loops[header][2].append(re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", re.sub(r"\.LBB\d+_\d+", ".LBB", t)))
    return [(loops[h][0], loops[h][2]) for h in order if loops[h][1]]


def short(name):
    try:
        return subprocess.check_output(["c++filt", name], text=True).strip().replace("(anonymous namespace)::", "").split("(")[0].replace("calitas::", "").replace("void ", "")
    except (OSError, subprocess.CalledProcessError):
        return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD~1", help="the revision to compare the working tree against")
    ap.add_argument("--show", action="store_true", help="print the diff of every kernel that differs")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "old"))
        os.makedirs(os.path.join(d, "new"))
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", a.rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", os.path.join(d, "old")], stdin=tar.stdout)
        if tar.wait() != 0:
            sys.exit("kernel_diff: git archive %s failed" % a.rev)
        old = functions_of(device_asm(os.path.join(d, "old", CSRC), os.path.join(d, "old")))
        new = functions_of(device_asm(os.path.join(ROOT, CSRC), os.path.join(d, "new")))
    bad = 0
    print("%-34s %-9s %-13s %-13s %-15s %s" % ("function", "code", "VGPR old/new", "SGPR old/new", "LDS old/new", "scratch, lane-shift loops old/new"))
    for name in sorted(set(old) | set(new), key=short):
        o, n = old.get(name), new.get(name)
        if o is None:                                           # a new kernel: its resources, nothing to compare
            print("%-34s new       VGPR %s  SGPR %s  LDS %s  scratch %s" % (short(name), n.get("vgpr", "-"), n.get("sgpr", "-"), n.get("lds", "-"), n.get("scratch", "-")))
            continue
        if n is None:
            print("%-34s only in %s" % (short(name), a.rev))
            bad += 1
            continue
        same = o["code"] == n["code"]
        bad += 0 if same else 1
        res = lambda k: "%s/%s" % (o.get(k, "-"), n.get(k, "-"))
        lo, ln = lane_shift_loops(o["raw"]), lane_shift_loops(n["raw"])
        print("%-34s %-9s %-13s %-13s %-15s %s, %s/%s%s" % (short(name), "identical" if same else "DIFFERS", res("vgpr"), res("sgpr"), res("lds"), res("scratch"),
                                                       [c for c, _ in lo], [c for c, _ in ln],
                                                       "" if same or not lo else " (the same but for register numbers)" if lo == ln else " (not the same)"))
        if not same and a.show:
            sys.stdout.writelines(x + "\n" for x in difflib.unified_diff(o["code"], n["code"], a.rev, "working tree", n=2, lineterm=""))
    print("%d of %d functions differ or are missing" % (bad, len(set(old) | set(new))))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
