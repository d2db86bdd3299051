"""-m "not gpu": the record of kernel builds (tests/golden/agreement_kernel_builds.json) stays in step with the library.  Every
kernel build (template instantiation) of libgnnpn_hip.so has one row: which GPU test files reach it (written by
tools/kernel_coverage.py from kernel traces) and the one test that compares this build's own output with a CPU reference — or a
waiver, for the few kernels that hand no numerical result to a caller.  A new instantiation without a row fails here."""
import ast
import importlib.util
import json
import os
import re

import pytest
import torch

from conftest import ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cov():
    import __graft_entry__ as entry
    tool = _tool()
    lib = entry.build()
    with open(tool.RECORD) as f:
        record = json.load(f)["builds"]
    return tool, tool.inventory(lib), record


def _gpu_tests(path):
    """{test function name: carries the gpu mark} of one test file, read from its source (nothing is imported or run)."""
    with open(path) as f:
        tree = ast.parse(f.read())

    def is_gpu_mark(node):
        return isinstance(node, ast.Attribute) and node.attr == "gpu" and isinstance(node.value, ast.Attribute) and node.value.attr == "mark"

    module_mark = False
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in node.targets):
            vals = node.value.elts if isinstance(node.value, (ast.List, ast.Tuple)) else [node.value]
            module_mark = any(is_gpu_mark(v) for v in vals)
    return {node.name: module_mark or any(is_gpu_mark(d) for d in node.decorator_list)
            for node in tree.body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}


def test_normalisation_of_kernel_names():
    tool = _tool()
    n = tool.normalise
    assert n("void (anonymous namespace)::csr_aggregate_tiled_kernel<10, 2, true>(HIP_vector_type<int, 2u> const*, int)") == \
        "csr_aggregate_tiled_kernel<10, 2, true>"
    assert n("__device_stub__linear_f32_kernel<128, 128>(float const*, long)") == "linear_f32_kernel<128, 128>"
    assert n("void lstm_encode_kernel<256,4>(LstmNets, int, int).kd") == "lstm_encode_kernel<256, 4>"
    assert n("pointer_decode_kernel<(int)32, (int)4, (bool)false>.kd") == "pointer_decode_kernel<32, 4, false>"
    assert n("void eswoa_kernel<RaggedT>(RaggedT, int const*)") == "eswoa_kernel<RaggedT>"
    assert n("(anonymous namespace)::dot_kernel(float const*, float const*, long, float*)") == "dot_kernel"
    assert tool.family("gemm_f32_kernel<true, false>") == "gemm_f32_kernel"


def test_every_build_has_a_row(cov):
    tool, builds, record = cov
    assert len(builds) == len(set(builds)) >= 100
    missing, stale = sorted(set(builds) - set(record)), sorted(set(record) - set(builds))
    assert not missing, f"kernel builds without a row in {os.path.relpath(tool.RECORD, ROOT)} (a new build needs a test and a row): {missing}"
    assert not stale, f"rows of builds that are no longer in the library: {stale}"


def test_every_row_names_a_gpu_test_that_reaches_it(cov):
    tool, builds, record = cov
    tests_of = {}
    for build in builds:
        row = record[build]
        assert ("checked_by" in row) != ("waived" in row), f"{build}: exactly one of checked_by / waived"
        assert all(os.path.exists(os.path.join(ROOT, t)) for t in row["reached_by"]), f"{build}: reached_by names a missing file"
        if "waived" in row:
            continue
        m = re.fullmatch(r"(tests/test_\w+\.py)::(test_\w+)(\[.+\])?", row["checked_by"])
        assert m, f"{build}: checked_by is no pytest node id: {row['checked_by']!r}"
        path, func = m.group(1), m.group(2)
        assert os.path.exists(os.path.join(ROOT, path)), f"{build}: {path} does not exist"
        if path not in tests_of:
            tests_of[path] = _gpu_tests(os.path.join(ROOT, path))
        assert func in tests_of[path], f"{build}: {path} has no test {func}"
        assert tests_of[path][func], f"{build}: {path}::{func} does not carry the gpu mark"
        assert path in row["reached_by"], f"{build}: no kernel trace of {path} shows this build (reached_by: {row['reached_by']})"


def test_waivers_are_few_and_only_for_kernels_without_a_result(cov):
    tool, builds, record = cov
    waived = [b for b in builds if "waived" in record[b]]
    assert len(waived) <= tool.MAX_WAIVED == 4, waived
    for b in waived:
        assert tool.family(b) in tool.NO_RESULT_KERNELS, f"{b} hands a result to its caller: it needs a checking test, not a waiver"
        assert isinstance(record[b]["waived"], str) and len(record[b]["waived"]) > 20, f"{b}: a waiver states its reason"


def test_the_tool_reports_nothing_open(cov):
    tool, builds, record = cov
    unreached, unchecked, stale = tool.problems({"builds": record}, builds)
    assert not unreached and not unchecked and not stale, (unreached, unchecked, stale)


def test_whh_split_operand_is_checked_before_any_launch():
    """ops.lstm_encode / ops.pointer_decode refuse a whh_split that is not the image pack_lstm_split_weights makes (the kernels read
    gnnpn_lstm_split_weights_bytes() bytes of it) before they touch any other operand: host tensors get that far."""
    from gnnpn_sc_amd import _lib, ops
    need = int(_lib.load().gnnpn_lstm_split_weights_bytes())
    assert need == 8 * 165888
    whh = torch.zeros(64, 4, 256, 4)
    assert ops.lstm_split_ptr(None, whh, "x") is None
    for bad in (torch.zeros(need - 1, dtype=torch.uint8), torch.zeros(need + 16, dtype=torch.uint8), torch.zeros(need, dtype=torch.int8),
                torch.zeros(need // 4), [0] * 8):
        with pytest.raises(ops.GnnpnError, match="whh_split.*image of pack_lstm_split_weights"):
            ops.lstm_split_ptr(bad, whh, "nets[0].whh_split")
    with pytest.raises(ops.GnnpnError, match="whh_split: on cpu, the weights it splits on meta"):
        ops.lstm_split_ptr(torch.zeros(need, dtype=torch.uint8), whh.to("meta"), "nets[0].whh_split")
    with pytest.raises(ops.GnnpnError, match="CUDA tensor"):            # right size, right device, but no device memory: dev_ptr's refusal
        ops.lstm_split_ptr(torch.zeros(need, dtype=torch.uint8), whh, "nets[0].whh_split")
    short = torch.zeros(need - 16, dtype=torch.uint8)
    enc = {"pregates": torch.zeros(1, 1, 1024), "whh": whh, "bhh": torch.zeros(1024), "whh_split": short}
    with pytest.raises(ops.GnnpnError, match="whh_split"):
        ops.lstm_encode([enc])
    z = torch.zeros(1)
    dec = {"enc_out": torch.zeros(1, 2, 256), "h0": z, "c0": z, "start": z, "wih": z, "whh": whh, "bih": z, "bhh": z, "whh_split": short}
    with pytest.raises(ops.GnnpnError, match="whh_split"):
        ops.pointer_decode([dec], torch.zeros(1, 2, 8), 1, 2)
