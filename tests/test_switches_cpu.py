"""CPU: vilco_amd/switches.py is the list of record of the VILCO_* switches.  Its table against the environment reads in the
sources (Python and csrc/), against the documents, and against ops.arithmetic_key(): every keyed entry moves the key, and the
keyed set is the one written out below."""
import glob
import os
import re

import pytest

from vilco_amd import _lib, ops, switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vilco_amd")
READ = re.compile(r'(?:getenv|vilco_env_flag|vilco_env_int|switches\.(?:on|text|number))\(\s*"(VILCO_[A-Z0-9_]+)"')

# what a captured step is keyed on (ops.arithmetic_key): dropping or adding one is an edit of this list
KEYED = ["_precision", "dw_precision", "DW_FAST_MIN_K", "producer_planes", "ln_planes", "attn_planes", "produce_amax",
         "conv_tap_planes", "defer_finish", "use_qkv_pre", "_FORKS", "_dw_fork_rows", "fold_skip_grads", "xl_ds_planes",
         "xl_scores_kernel", "linear_group_enabled", "use_flash", "_reuse_packs", "_weight_cache", "range_check",
         "vilco_gemm_config_gen()", "pack_group_enabled", "conv_dz_planes", "ln_bwd_amax", "fused_prompt"]
UNSET = ["_precision", "DW_FAST_MIN_K", "vilco_gemm_config_gen()"]        # the pieces of the key that no variable sets


def _sources():
    py = [p for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)]
    return py, glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))


def _reads():
    """{variable: files (relative to vilco_amd/) that read it}"""
    found = {}
    for p in sum(_sources(), []):
        with open(p) as f:
            for name in READ.findall(f.read()):
                found.setdefault(name, set()).add(os.path.relpath(p, PKG))
    return found


def _reader_file(reader):
    if reader.endswith((".hip", ".h")):
        return os.path.join("csrc", reader)
    if reader.startswith("PtTransformer."):
        return os.path.join("modeling", "meta_archs.py")
    parts = reader.split(".")
    return next(os.path.join(*parts[:n]) + ".py" for n in range(len(parts), 0, -1)
                if os.path.exists(os.path.join(PKG, *parts[:n]) + ".py"))


def test_table_matches_the_source():
    envs = [s.env for s in switches.TABLE if s.env is not None]
    assert len(envs) == len(set(envs)), "a variable is declared twice"
    found = _reads()
    assert set(found) == set(envs)
    for s in switches.TABLE:
        if s.env is not None:
            assert found[s.env] == {_reader_file(r) for r in s.readers}, s.env
    # Python reads no VILCO_* variable past the three readers
    for p in _sources()[0]:
        with open(p) as f:
            assert not re.search(r'environ[^\n]*"VILCO_', f.read()), p


def test_table_matches_the_documents():
    text = ""
    for doc in ("INTEGRATION.md", "README.md"):
        with open(os.path.join(ROOT, doc)) as f:
            text += f.read()
    documented = set(re.findall(r"VILCO_[A-Z0-9_]+", text))
    assert not [s.env for s in switches.TABLE if s.env is not None and s.env not in documented]


def test_every_row_says_why_it_is_keyed_or_not():
    for s in switches.TABLE:
        assert isinstance(s.default, str) and s.readers and s.key and s.meaning, s
        if s.key == switches.KEYED:
            assert any(r.startswith("ops.") for r in s.readers), s


def test_keyed_set_is_frozen():
    assert len(set(switches.KEYED_OPS)) == len(switches.KEYED_OPS)
    assert set(switches.KEYED_OPS) | set(UNSET) == set(KEYED) and not set(switches.KEYED_OPS) & set(UNSET)
    assert len(ops.arithmetic_key()) == len(KEYED)


def _other(v):
    if isinstance(v, bool):
        return not v
    if isinstance(v, set):
        return v ^ {"dw"}
    if isinstance(v, str):
        return "warn" if v != "warn" else "auto"
    return 4 if v is None else v + 1


@pytest.mark.parametrize("name", KEYED)
def test_every_keyed_entry_moves_the_key(name):
    first = ops.arithmetic_key()
    hash(first)                                          # graph.GraphedStep uses it inside a dict key
    if name == "vilco_gemm_config_gen()":                # a generation: it only rises, there is no way back
        lib = _lib.load()
        assert lib.vilco_gemm_force(0, 0) == 0           # the configuration it already has
        assert ops.arithmetic_key() != first
        return
    if name == "_precision":
        saved = ops.get_precision()
        try:
            ops.set_precision((saved + 1) % 4)
            assert ops.arithmetic_key() != first
        finally:
            ops.set_precision(saved)
        assert ops.arithmetic_key() == first
        return
    saved = getattr(ops, name)
    try:
        setattr(ops, name, _other(saved))
        assert ops.arithmetic_key() != first
    finally:
        setattr(ops, name, saved)
    assert ops.arithmetic_key() == first


def test_readers_follow_the_environment_and_fall_back_to_the_declared_default(monkeypatch):
    for env in ("VILCO_XL_DS_PLANES", "VILCO_RANGE_CHECK", "VILCO_DW_FORK_ROWS", "VILCO_DP_GRAPH_COMM"):
        monkeypatch.delenv(env, raising=False)
    assert switches.on("VILCO_XL_DS_PLANES") is True and switches.on("VILCO_DP_GRAPH_COMM") is False
    assert switches.text("VILCO_RANGE_CHECK") == "0" and switches.number("VILCO_DW_FORK_ROWS") == 0
    monkeypatch.setenv("VILCO_XL_DS_PLANES", "0")
    monkeypatch.setenv("VILCO_RANGE_CHECK", "auto")
    monkeypatch.setenv("VILCO_DW_FORK_ROWS", "288")
    assert switches.on("VILCO_XL_DS_PLANES") is False
    assert switches.text("VILCO_RANGE_CHECK") == "auto" and switches.number("VILCO_DW_FORK_ROWS") == 288
    for spelling in ("", "1", "00", "off", "false"):            # everything but "0" is on
        monkeypatch.setenv("VILCO_XL_DS_PLANES", spelling)
        assert switches.on("VILCO_XL_DS_PLANES") is True


@pytest.mark.parametrize("reader", [switches.on, switches.text, switches.number])
def test_an_undeclared_name_raises(reader, monkeypatch):
    monkeypatch.setenv("VILCO_NOT_A_SWITCH", "1")              # set or not: it has to be in the table
    with pytest.raises(KeyError):
        reader("VILCO_NOT_A_SWITCH")
