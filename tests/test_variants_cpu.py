"""Keeps the GPU suite complete over what the library can select (no GPU needed: source files are read, nothing is launched).

Two lists are taken from the library's own sources and held against the string literals of tests/test_gpu_*.py (docstrings and
comments do not count: a name has to be something a test passes to set_tuning / tuning= or compares last_dispatch() with):
  * every laboratory key of ofdm_amd/csrc/ofdm_hip_tuning.h that the product build accepts selects a kernel, a grid shape or a
    chunking that some GPU test must have run -- or is listed in MEASUREMENT_ONLY with the reason why no result depends on it;
  * every dispatch name a launcher can append to ofdm_last_dispatch -- the literals on the trace_add( lines under ofdm_amd/csrc/ and
    the names[] table kernels_sym.hip indexes -- must be a name some GPU test expects, so that a launcher change that stops reaching
    a kernel fails a test; or it is listed in UNREACHABLE with the reason why no ABI call can produce it.
tests/test_gpu_variants.py holds the cases for the variants that only a key or a batch shape selects."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofdm_amd", "csrc")

# keys whose setting changes no delivered result: nothing to compare with a reference
MEASUREMENT_ONLY = {
    "chest_solve_only": "ofdm_chest_smooth_batch then launches k_chest_solve alone into its workspace and delivers nothing",
}
# dispatch names no ABI call can produce
UNREACHABLE = {
    "k_rxframe64<list>": "run_rxframe64 takes a caller's frame list only from the one-pass receive path, which is gone: its one "
                         "caller (ofdm_abi.hip, the N = 64 decode chain) passes no list",
}


def lab_keys():
    """[(key, profile_build_only)] of ofdm_hip_tuning.h"""
    txt = open(os.path.join(CSRC, "ofdm_hip_tuning.h")).read()
    return [(k, prof == "true") for k, prof in re.findall(r'^OFDM_TUNE_KEY\("([a-z0-9_]+)",\s*\w+,\s*(true|false)\)', txt, re.M)]


def dispatch_names():
    """{name: where} of every kernel name a launcher can append to the dispatch trace ('a+b' literals count as a and b)"""
    names = {}
    for path in sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)):
        lines = open(path).read().splitlines()
        for i, line in enumerate(lines):
            if "trace_add(" not in line or line.lstrip().startswith(("//", "inline")):
                continue
            lits = re.findall(r'"([^"]*)"', line.split("trace_add(", 1)[1])
            if not lits:                                   # trace_add(p.trace, names[MODE]): the table it indexes
                table = re.search(r"trace_add\([^,]+,\s*(\w+)\[", line).group(1)
                decl = next(l for l in lines[:i][::-1] if re.search(r"\b%s\[\]\s*=" % table, l))
                lits = re.findall(r'"([^"]*)"', decl)
            assert lits, (path, i + 1)
            for lit in lits:
                for name in lit.split("+"):
                    names.setdefault(name, "%s:%d" % (os.path.basename(path), i + 1))
    return names


def gpu_test_literals(exclude=()):
    """every string literal of tests/test_gpu_*.py that is not a docstring, whole and split at '+' (dispatch strings join names so)"""
    out = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        if os.path.basename(path) in exclude:
            continue
        tree = ast.parse(open(path).read())
        doc = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.Module, ast.FunctionDef, ast.ClassDef)) and node.body and isinstance(node.body[0], ast.Expr) \
                    and isinstance(node.body[0].value, ast.Constant):
                doc.add(id(node.body[0].value))
        for node in ast.walk(tree):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and id(node) not in doc:
                out.add(node.value)
                out.update(node.value.split("+"))
    return out


def missing_keys(literals):
    return [k for k, prof in lab_keys() if not prof and k not in MEASUREMENT_ONLY and k not in literals]


def missing_dispatch_names(literals):
    return {n: where for n, where in dispatch_names().items() if n not in UNREACHABLE and n not in literals}


def test_the_parsers_see_the_sources():
    keys = dict(lab_keys())
    assert len(keys) >= 30 and keys["fcs_bitserial"] is False and keys["debug_sc"] is True
    assert {k for k, prof in keys.items() if prof} == {"debug_demod64", "debug_sc", "debug_tx"}   # profile build only: not in the product
    names = dispatch_names()
    for n in ("k_sym<fft>", "k_sym<llr>", "k_demod64<burst8>", "k_sc_tile<list,cross>", "k_sc_tile<list,peak>", "k_sc_stream<regs>",
              "k_txframe_mid<rewrite>", "k_scb_fine<5>", "k_rxframe64<cut,list>", "k_sc80"):
        assert n in names, n
    assert len(names) >= 40 and all(re.fullmatch(r"k_[a-z0-9_]+(<[a-z0-9_,]+>)?", n) for n in names), sorted(names)
    lits = gpu_test_literals()
    assert "k_sc80" in lits and "no_sc80" in lits and "k_sc_cf<256,list>" in lits
    assert "the same rows" not in " ".join(l for l in lits if len(l) > 60)     # docstrings stay out (tests/chain_checks.py wording)


def test_every_laboratory_key_is_run_by_a_gpu_test():
    keys = [k for k, _ in lab_keys()]
    assert set(MEASUREMENT_ONLY) <= set(keys), "MEASUREMENT_ONLY names a key the library no longer has"
    missing = missing_keys(gpu_test_literals())
    assert not missing, f"laboratory keys no GPU test sets: {missing} (tests/test_gpu_variants.py, or MEASUREMENT_ONLY with a reason)"


def test_every_dispatch_name_is_expected_by_a_gpu_test():
    assert set(UNREACHABLE) <= set(dispatch_names()), "UNREACHABLE names a kernel no launcher traces any more"
    missing = missing_dispatch_names(gpu_test_literals())
    assert not missing, f"dispatch names no GPU test expects: {missing} (assert it where the kernel is run, or UNREACHABLE with a reason)"
