#!/usr/bin/env python3
"""Compare device assembly per kernel: tools/asm_kernels.py OLD.s NEW.s [NEW2.s ...]

OLD and NEW are files written by `make -C csrc asm` in two trees.  Every kernel of the NEW
files is looked up by symbol in OLD and two things are compared: the function body and the
.amdhsa_kernel descriptor block (VGPRs, SGPRs, scratch, LDS).  For code that moved between
units, where the whole-file hashes cannot match.  Basic-block labels carry the function's
index within its file (.LBB7_3), so they are renumbered, and the column padding before the
compiler's comments is collapsed; nothing else is normalised."""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    """{symbol: {"body": text, "desc": text}} of one .s file"""
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        j = i
        while not re.match(r"\.Lfunc_end\d+:", lines[j]):
            j += 1
        chunk = lines[i:j]
        k = {}
        k0 = next((n for n, l in enumerate(chunk) if ".amdhsa_kernel" in l), None)
        if k0 is not None:
            k1 = next(n for n, l in enumerate(chunk) if ".end_amdhsa_kernel" in l)
            k["desc"] = "\n".join(chunk[k0:k1])
            chunk = chunk[:k0]
        chunk = [re.sub(r"BB\d+_(\d+)", r"BB_\1", re.sub(r"\s+", " ", l)) for l in chunk]
        k["body"] = "\n".join(chunk)
        out[m.group(1)] = k
        i = j
    return out


def demangle(sym):
    d = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    return d.replace("msfno::(anonymous namespace)::", "")[:90]


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old = kernels(argv[1])
    seen, differ = set(), 0
    for path in argv[2:]:
        for sym, k in kernels(path).items():
            if "desc" not in k:
                continue  # a device function, not a kernel
            seen.add(sym)
            o = old.get(sym)
            if o is None:
                verdict = "not in OLD"
            else:
                same_b, same_d = o["body"] == k["body"], o.get("desc") == k["desc"]
                verdict = ("body same" if same_b else "BODY DIFFERS") + ", " + \
                          ("descriptor same" if same_d else "DESCRIPTOR DIFFERS")
                differ += not (same_b and same_d)
            h = hashlib.sha256(k["body"].encode()).hexdigest()[:12]
            print(f"{path.split('/')[-1]:<22} {h}  {verdict:<36} {demangle(sym)}")
    for sym, k in old.items():
        if "desc" in k and sym not in seen:
            print(f"only in OLD: {demangle(sym)}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
