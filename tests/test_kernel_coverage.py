"""CPU-only guard: every exported `mp_*` entry point of include/medplib_hip.h is exercised by some tests/test_gpu_*.py, by its own
name or through a Python wrapper that calls it, unless it is listed in ALLOW with a reason.  The wrappers are read from
medplib_amd/ops.py and from the other host modules that call the library directly (preprocess, tail_program, comm, ...).

Also here: the crafted MoE routing cases of the backward parity tests are checked on the CPU to contain every drop pattern."""
import ast
import glob
import os
import re

import torch

from kernel_parity import drop_patterns, moe_cases, route_top1_cpu, route_top2_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> why no single-GPU test can or need call it.  Nothing here computes or moves tensor data on one GPU.
ALLOW = {
    "mp_version": "version number, no device work (test_abi.py reads it)",
    "mp_arch": "architecture string, no device work (build() checks it)",
    "mp_last_error_string": "error string of the last failed call, no device work",
    "mp_profile_marker": "empty marker kernel for profiler traces, computes nothing",
    "mp_gemm_fold_ok": "host-only predicate on a GEMM shape",
    "mp_gemm_set_stream_workspace": "workspace registration for a side stream, no kernel",
    "mp_pil_bilinear_ksize": "host-only: size of a resampling coefficient table (tests/test_preprocess.py)",
    "mp_pil_bilinear_coeffs": "host-only: resampling coefficients computed on the CPU (tests/test_preprocess.py)",
    "mp_pil_resample_ksize": "host-only: size of a resampling coefficient table (tests/test_rag_host.py)",
    "mp_pil_resample_coeffs": "host-only: resampling coefficients computed on the CPU (tests/test_rag_host.py)",
    "mp_comm_unique_id_bytes": "RCCL bootstrap, needs more than one rank",
    "mp_comm_unique_id": "RCCL bootstrap, needs more than one rank",
    "mp_comm_init": "RCCL communicator, needs more than one rank",
    "mp_comm_destroy": "RCCL communicator, needs more than one rank",
    "mp_comm_count": "RCCL communicator, needs more than one rank",
    "mp_alltoallv_tokens": "RCCL point-to-point exchange, needs more than one rank",
}


def exported_names():
    src = open(os.path.join(ROOT, "include", "medplib_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b(mp_\w+)\s*\(", src)))


def _functions(path):
    """{name: source} for the module's top-level functions, {Class.method: source} for its classes' methods; a class with forward and
    backward (a torch.autograd.Function) also gets Class.apply = both, since `Class.apply(...)` is how a test runs its backward."""
    src = open(path).read()
    out = {}
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            out[node.name] = ast.get_source_segment(src, node)
        elif isinstance(node, ast.ClassDef):
            meth = {sub.name: ast.get_source_segment(src, sub) for sub in node.body if isinstance(sub, ast.FunctionDef)}
            for m, text in meth.items():
                out[node.name + "." + m] = text
            if "forward" in meth and "backward" in meth:
                out[node.name + ".apply"] = meth["forward"] + "\n" + meth["backward"]
    return out


def _call_pattern(name):
    """How a call of a wrapper looks: `name(` for a function, `.method(` for Class.method."""
    if "." in name:
        return r"\.%s\s*\(" % re.escape(name.split(".", 1)[1])
    return r"\b%s\s*\(" % re.escape(name)


def _wrapper_called(w, text):
    """A function wrapper: `w(` appears.  A method wrapper Class.method: the text names the class and calls `.method(` (a bare
    `.forward(` or `.call(` of something else does not count)."""
    if "." in w:
        cls = w.split(".", 1)[0]
        return bool(re.search(r"\b%s\b" % re.escape(cls), text) and re.search(_call_pattern(w), text))
    return bool(re.search(_call_pattern(w), text))


def wrapper_map():
    """{mp_name: set of Python wrappers (function or Class.method) that reach it}, following calls between the package's functions."""
    fns = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "medplib_amd", "**", "*.py"), recursive=True)):
        for f, text in _functions(path).items():
            fns[f] = fns.get(f, "") + "\n" + text                       # the same name in two modules: either may be meant
    direct = {f: set(re.findall(r"""["'](mp_\w+)["']""", s)) | set(re.findall(r"_raw_(mp_\w+)", s)) for f, s in fns.items()}
    def reaches(f, text, g):
        if "." in f and "." in g and f.split(".", 1)[0] == g.split(".", 1)[0]:          # a method calling its own class's method
            return bool(re.search(r"\bself\.%s\s*\(" % re.escape(g.split(".", 1)[1]), text))
        return _wrapper_called(g, text)
    calls = {f: {g for g in fns if g != f and reaches(f, s, g)} for f, s in fns.items()}
    changed = True
    while changed:
        changed = False
        for f in fns:
            for g in calls[f]:
                new = direct[g] - direct[f]
                if new:
                    direct[f] |= new
                    changed = True
    reach = {}
    for f, names in direct.items():
        if f.split(".")[-1].startswith("__"):
            continue
        for n in names:
            reach.setdefault(n, set()).add(f)
    return reach


def _code_only(path):
    """The file's code without comments and docstrings (a name mentioned in prose does not count as a call)."""
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        body = getattr(node, "body", None)
        if isinstance(body, list) and body and isinstance(body[0], ast.Expr) and isinstance(getattr(body[0], "value", None), ast.Constant) \
                and isinstance(body[0].value.value, str):
            body[0] = ast.Pass()
    return ast.unparse(tree)


def gpu_test_files():
    return {p: _code_only(p) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))}


def uncovered():
    files, wrap = gpu_test_files(), wrapper_map()
    out = []
    for n in exported_names():
        if any(re.search(r"\b%s\b" % n, t) for t in files.values()):
            continue
        if any(_wrapper_called(w, t) for w in wrap.get(n, ()) for t in files.values()):
            continue
        out.append(n)
    return out


def test_every_entry_point_is_called_by_a_gpu_test():
    names = exported_names()
    assert len(names) > 100, "the header parse found too few entry points"
    missing = [n for n in uncovered() if n not in ALLOW]
    assert not missing, "entry points no tests/test_gpu_*.py calls (add a parity test, not an allowlist entry): " + ", ".join(missing)


def test_allowlist_is_tight():
    names = set(exported_names())
    stale = sorted(set(ALLOW) - names)
    assert not stale, f"allowlist names the header does not export: {stale}"
    for n, why in ALLOW.items():
        assert why.strip(), n
    # single-GPU tensor kernels carry their element type in the name; nothing of that kind may be excused
    kinds = ("host-only", "RCCL", "no device work", "computes nothing", "no kernel")
    for n, why in ALLOW.items():
        assert any(k in why for k in kinds), f"{n}: the reason must be one of {kinds}"
        if re.search(r"_(bf16|f32|u8)$", n):
            assert "RCCL" in why, f"{n} looks like a tensor kernel: it needs a test, not an excuse"


def test_prose_and_generic_method_names_do_not_count():
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write('"""mp_sumsq_accum_f32 in a docstring"""\n# mp_adamw_step_f32 in a comment\ndef t():\n    "mp_mean_plus_f32"\n    x.forward(1)\n')
    try:
        code = _code_only(f.name)
    finally:
        os.unlink(f.name)
    assert "mp_" not in code
    assert not _wrapper_called("TailProgram.forward", code) and _wrapper_called("t", "t (1)")


def test_parse_sees_the_wrappers():
    wrap = wrapper_map()
    assert "sumsq_accum" in wrap["mp_sumsq_accum_f32"]
    assert {"gather_rows_bf16", "scatter_rows_bf16_"} <= wrap["mp_gather_rows_bf16"]
    assert "mp_adamw_step_f32" in exported_names()


def test_crafted_routing_cases_hold_every_drop_pattern():
    seen2, seen1, experts = set(), set(), set()
    empty_expert = False
    for name, E, cap, logits, gates in moe_cases():
        T = gates.shape[0]
        experts.add(E)
        expert, slot, weight, tot1 = route_top2_cpu(gates, logits, cap)
        pats = drop_patterns(slot, T)
        seen2 |= pats
        named = torch.bincount(expert.long(), minlength=E)
        empty_expert |= bool((named == 0).any())
        e1, s1, w1, c1 = route_top1_cpu(gates, cap)
        seen1 |= {"kept"} if bool((s1 >= 0).any()) else set()
        seen1 |= {"dropped"} if bool((s1 < 0).any()) else set()
        if name == "e4_all_patterns":
            assert pats == {"none", "first_only", "second_only", "both"}, pats
        if name == "e4_no_drops":
            assert pats == {"none"} and bool((s1 >= 0).all())
        # kept weights of a token sum to 1, a token with both choices dropped has weight 0 (the D <= eps clamp)
        k1, k2 = slot[:T] >= 0, slot[T:] >= 0
        tot = weight[:T] + weight[T:]
        assert torch.allclose(tot[k1 | k2], torch.ones(int((k1 | k2).sum()), dtype=torch.float64))
        assert bool((tot[~k1 & ~k2] == 0).all())
    assert seen2 == {"none", "first_only", "second_only", "both"}
    assert seen1 == {"kept", "dropped"}
    assert empty_expert and experts == {2, 4, 8}
