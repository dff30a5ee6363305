#!/usr/bin/env python3
"""Device-code diff of libfgcn against another revision (no GPU needed): every csrc/*.hip of the working tree and of REV is compiled
to gfx950 assembly and compared kernel by kernel.  Prints, per source, the kernels whose text differs or that exist on one side
only; exits non-zero if there are any.  A refactor that only moves helpers must come out empty.

    python tools/kdiff.py REV [stem ...]        # e.g. HEAD~ ; stems as for kres.py (joint, tconv, ...), default: all
"""
import glob
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

from kres import FLAGS, ROOT, demangle, device_asm, kernels

CSRC = os.path.join("fusion_gcn_amd", "csrc")


def tree_kernels(root, name):
    """One source of the tree at `root` -> its kernels, without the __hip_cuid_* lines (they differ between any two compiles), without
    comments, and with the function's index taken out of its local labels (.LBB12_3 -> .LBB_3: the index is the order in which the
    host code names the kernels, not device code)."""
    src = os.path.join(root, CSRC, name)
    if not os.path.exists(src):
        return {}
    flags = [f for f in FLAGS if not f.startswith("-I")] + [f"-I{root}/include"]
    lines = [re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", l.split(";")[0].rstrip()) for l in device_asm(src, flags) if "__hip_cuid_" not in l]
    return kernels([l for l in lines if l])


def main():
    rev, stems = sys.argv[1], sys.argv[2:]
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        names = sorted({os.path.basename(p) for r in (ROOT, old) for p in glob.glob(os.path.join(r, CSRC, "*.hip"))})
        if stems:
            names = [n for n in names if n[5:-4] in stems]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
            new_k = ex.map(lambda n: tree_kernels(ROOT, n), names)
            old_k = ex.map(lambda n: tree_kernels(old, n), names)
            pairs = list(zip(names, old_k, new_k))
    bad = 0
    for name, a, b in pairs:
        findings = [("differs", k) for k in a if k in b and a[k] != b[k]]
        findings += [(f"only in {rev}", k) for k in a if k not in b] + [("only in the working tree", k) for k in b if k not in a]
        print(f"{name}: {len(a)} kernels in {rev}, {len(b)} here, {len(findings)} findings")
        for what, k in findings:
            print(f"    {what}: {demangle(k)}")
        bad += len(findings)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
