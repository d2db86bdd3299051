"""The patched copy of csrc/ the ablation tools (ablate_aggregate.py, ablate_gin_layer.py) compile their timing-only builds from: the
product sources carry no experiment switch, tools/experiments/<patch> adds them to a copy."""
import os, re, shutil, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gnnpn-sc_amd")
OUT = os.path.join(PKG, "build", "ablate")

# the commit whose sources a frozen patch applies to (later kernels moved on)
BASE = {"aggregate_switches.patch": "76d19b13d7", "aggregate_prefetch_wave.patch": "f5daec2", "gin_layer_split_switches.patch": "b4df9ef",
        "aggregate_stamps.patch": "361441c", "aggregate_fill_tokens.patch": "361441c"}


def patched_csrc(patch):
    """A copy of csrc/ (+ include/) with tools/experiments/<patch> applied; returns the copy's csrc directory.  A patch listed in
    BASE is frozen: the files it touches are taken from that commit (``git show``; needs the repository, i.e. build here, run on
    the GPU box)."""
    dst = os.path.join(OUT, "src_" + patch.replace(".patch", ""))
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(os.path.join(dst, "gnnpn-sc_amd"), exist_ok=True)
    shutil.copytree(os.path.join(PKG, "csrc"), os.path.join(dst, "gnnpn-sc_amd", "csrc"))
    ppath = os.path.join(ROOT, "tools", "experiments", patch)
    if patch in BASE:
        for f in sorted(set(re.findall(r"^\+\+\+ [ab]/(\S+)", open(ppath).read(), re.M))):
            blob = subprocess.run(["git", "show", f"{BASE[patch]}:{f}"], check=True, cwd=ROOT, capture_output=True).stdout
            os.makedirs(os.path.dirname(os.path.join(dst, f)), exist_ok=True)    # (a frozen patch may also touch the header, the oracle, a test)
            open(os.path.join(dst, f), "wb").write(blob)
    subprocess.run(["git", "apply", "--unsafe-paths", "--directory=" + dst, ppath], check=True, cwd=ROOT)
    return os.path.join(dst, "gnnpn-sc_amd", "csrc")
