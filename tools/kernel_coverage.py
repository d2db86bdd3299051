"""Which kernel builds libgnnpn_hip.so holds, and which GPU test files reach each of them (host only).

    python tools/kernel_coverage.py inventory                 # the builds of the linked library, one per line
    python tools/kernel_coverage.py update --trace DIR        # rewrite every reached_by of the record from kernel traces
    python tools/kernel_coverage.py report                    # unreached / unchecked builds of the record; exit 1 if any

Inventory: every kernel (template instantiation) leaves one weak host stub ``__device_stub__<name>(<args>)`` in the linked
library; ``nm -C`` lists them.  A build's name is the demangled stub without the prefix, the ``(anonymous namespace)::``
qualifiers, a leading ``void `` and the argument list, with one spelling of the template arguments (``<256, 4, false>``).

Trace: DIR holds the ``*kernel_stats.csv`` files of ``rocprofv3 --kernel-trace --stats --output-format csv`` runs, one run per
GPU test file, each file named ``<test file stem>.<n>.kernel_stats.csv`` (n: one per traced process).  The kernel names in
them go through the same normalisation (plus a ``.kd`` suffix dropped).  A traced name whose family is one of the library's
but which is no build of the inventory is an error: the normalisation, or the record, is out of date.

The record is tests/golden/agreement_kernel_record_tabu_pairs.json: per build ``reached_by`` (written here) and ``checked_by`` (one pytest
node id whose test compares this build's own output with a CPU reference) or ``waived`` (a reason; only for kernels that hand
no numerical result to a caller).  tests/test_kernel_inventory_host.py keeps the record and the library in step; it reads the
record at RECORD below.  (Committed golden files are never edited, so a pull request that adds a kernel build continues the record in
a new file: tests/golden/agreement_kernel_builds.json is the record as it stood before the descent kernels,
agreement_kernel_record.json as it stood before multi-start descent (descend_select_kernel),
agreement_kernel_record_multistart.json as it stood before pair-swap descent (descend_pairs_kernel),
agreement_kernel_record_pairs.json as it stood before its workgroup form (descend_pairs_wide_kernel),
agreement_kernel_record_pairs_window.json as it stood before the shortlist builds (descend_pairs_shortlist_kernel,
descend_pairs_shortlist_wide_kernel), agreement_kernel_record_pairs_shortlist.json as it stood before the service ids
(woa_services_kernel, search_services_kernel, services_merit_kernel, services_merit_wide_kernel),
agreement_kernel_record_services.json as it stood before the four pointer_decode_glimpse_kernel builds got a checking test of their
own (checked_by moved from the end-to-end attention fixtures to test_attention_decode_build_vs_float64_replay, no new build),
agreement_kernel_record_attn_decode.json as it stood before score_select_kernel, agreement_kernel_record_score_select.json as it
stood before pick_prob_kernel, the ten pointer_decode_lean_kernel builds and the two pointer_decode_coop_kernel builds got checking
tests of their own (checked_by moved from test_two_level_greedy_golden and test_pointer_decode_cooperative_build to
tests/test_gpu_decode_replay.py, no new build), agreement_kernel_record_decode_replay.json as it stood before the tabu walk
(descend_tabu_kernel, descend_tabu_wide_kernel), agreement_kernel_record_tabu.json as it stood before the walk over pair moves
(descend_tabu_pairs_kernel, descend_tabu_pairs_wide_kernel); the current record repeats every row of its predecessors, with
reached_by grown by the new GPU test file where there is one; nothing reads the eleven older files.)
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gnnpn-sc_amd", "libgnnpn_hip.so")
RECORD = os.path.join(ROOT, "tests", "golden", "agreement_kernel_record_tabu_pairs.json")
NO_RESULT_KERNELS = ("lds_interferer_kernel", "gate_wait_kernel", "coop_zero_kernel")   # hand no numerical result to a caller
MAX_WAIVED = 4


def _cut_arguments(name):
    """'f<a, (b)1>(int, g<h>(*)(x))' -> 'f<a, (b)1>': cut at the first '(' outside every <...>."""
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


def normalise(name):
    """One spelling for a kernel build, from a demangled stub symbol or from a profiler's kernel name."""
    name = name.strip()
    if name.endswith(".kd"):
        name = name[:-3]
    name = name.replace("__device_stub__", "").replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    name = _cut_arguments(name).strip()
    if "<" in name:
        base, args = name.split("<", 1)
        args = args.rsplit(">", 1)[0]
        parts = []
        for a in args.split(","):
            a = re.sub(r"^\((int|bool|unsigned int|unsigned|long)\)", "", a.strip())   # '(bool)1' / '(int)256' spellings
            parts.append(a)
        name = base.strip() + "<" + ", ".join(parts) + ">"
    return name


def family(build):
    return build.split("<", 1)[0]


def inventory(lib=LIB):
    """Sorted names of the kernel builds in the linked library."""
    out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        if "__device_stub__" not in line:
            continue
        sym = line.split(None, 2)[2] if re.match(r"^[0-9a-fA-F]+\s+\S\s", line) else line.split(None, 1)[1]
        names.add(normalise(sym))
    return sorted(names)


def traced_names(stats_csv):
    """Kernel names of one *kernel_stats.csv (column 'Name')."""
    with open(stats_csv, newline="") as f:
        rows = list(csv.DictReader(f))
    return [r["Name"] for r in rows if r.get("Name")]


def reached_by(trace_dir, builds):
    """{build: sorted test files whose trace shows it}; raises on a traced kernel of a known family that is no known build."""
    builds = set(builds)
    families = {family(b) for b in builds}
    reached = {b: set() for b in builds}
    unknown = []
    files = sorted(glob.glob(os.path.join(trace_dir, "*.kernel_stats.csv")))
    if not files:
        raise SystemExit(f"no *.kernel_stats.csv under {trace_dir}")
    for path in files:
        test_file = "tests/" + os.path.basename(path).split(".", 1)[0] + ".py"
        for raw in traced_names(path):
            n = normalise(raw)
            if n in builds:
                reached[n].add(test_file)
            elif family(n) in families or "gnnpn" in raw:
                unknown.append((test_file, raw, n))
    if unknown:
        lines = "\n".join(f"  {t}: {raw!r} -> {n!r}" for t, raw, n in unknown[:20])
        raise SystemExit(f"{len(unknown)} traced kernel names of this library's families match no build of the inventory:\n{lines}")
    return {b: sorted(v) for b, v in reached.items()}


def load_record(path=RECORD):
    with open(path) as f:
        return json.load(f)


def save_record(rec, path=RECORD):
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def problems(rec, builds):
    """(unreached, unchecked, stale): builds that are not waived and that no trace shows / that name no checking test /
    rows of the record that are no build any more (and builds without a row)."""
    rows = rec["builds"]
    unreached = [b for b in builds if b in rows and "waived" not in rows[b] and not rows[b].get("reached_by")]
    unchecked = [b for b in builds if b in rows and "waived" not in rows[b] and not rows[b].get("checked_by")]
    stale = sorted(set(rows) ^ set(builds))
    return unreached, unchecked, stale


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("command", choices=["inventory", "update", "report"])
    ap.add_argument("--lib", default=LIB)
    ap.add_argument("--record", default=RECORD)
    ap.add_argument("--trace", help="directory of <test file stem>.<n>.kernel_stats.csv files (update)")
    ap.add_argument("--only", nargs="*", default=None,
                    help="update: replace only these test files' entries (tests/x.py ...), keep what the record holds of the others")
    a = ap.parse_args(argv)
    builds = inventory(a.lib)
    if a.command == "inventory":
        print("\n".join(builds))
        print(f"{len(builds)} builds in {len({family(b) for b in builds})} families", file=sys.stderr)
        return 0
    rec = load_record(a.record) if os.path.exists(a.record) else {"builds": {}}
    if a.command == "update":
        if not a.trace:
            ap.error("update needs --trace DIR")
        got = reached_by(a.trace, builds)
        traced_files = {t for v in got.values() for t in v} if a.only is None else set(a.only)
        for b in builds:
            row = rec["builds"].setdefault(b, {})
            kept = [t for t in row.get("reached_by", []) if t not in traced_files] if a.only is not None else []
            row["reached_by"] = sorted(set(kept) | set(got[b]))
        for b in sorted(set(rec["builds"]) - set(builds)):
            del rec["builds"][b]                      # a build that left the library leaves the record
        save_record(rec, a.record)
    unreached, unchecked, stale = problems(rec, builds)
    waived = [b for b in builds if "waived" in rec["builds"].get(b, {})]
    print(f"{len(builds)} builds, {len(waived)} waived, {len(unreached)} unreached, {len(unchecked)} unchecked, "
          f"{len(stale)} rows out of step with the library")
    for title, names in (("unreached", unreached), ("unchecked", unchecked), ("out of step", stale)):
        for n in names:
            print(f"  {title}: {n}")
    return 1 if (unreached or unchecked or stale) else 0


if __name__ == "__main__":
    sys.exit(main())
