"""The finalized BatchNorm tables in the engine's launch plans, built on the
host (no GPU): realnvp_hip/engine.py alloc_saved / _fwd_args / _bwd_args with
engine.BN_TABLES, for the shapes of test_fold_plan_cpu.py.

Checks: every backward BatchNorm source of a training plan whose launches the
table shortens (data-gradient epilogues, folded and standalone BatchNorm
backward) points at its BatchNorm's slot of the saved arena's table region,
16-byte aligned; the tables of distinct BatchNorms do not overlap and lie
outside the byte range the end of a step zeroes; the running-statistics
update (the writer) has one row per BatchNorm with the same destination;
forward sources, eval plans and BN_TABLES = False carry NULL -- and so do the
weight-gradient prologues, which keep the shard reduction (measured: their
launches do not get shorter with a table, profiles/bn_tables_kernels.txt).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dl-normalizing-flows_amd"))

from test_fold_plan_cpu import CASES  # noqa: E402


def _engine(kind, cio, mid, size):
    import modules_realnvp as MR
    import utils
    hp = utils.Hyperparameters(32, 4, True, True, True, True)
    torch.manual_seed(0)
    mod = MR.CheckerboardAffineCoupling(cio, mid, size, 1.0, hp) if kind == "ckbd" else \
        MR.ChannelwiseAffineCoupling(cio, mid, 0.0, hp)
    return mod.engine()


def _bwd_sources(items, groups):
    """(what, BNSrc) of every BatchNorm source of a backward plan."""
    out = []
    for kind, c, nb, fl, bn, rw in items:
        if kind == "dgrad":
            if c.epi_relu_bn_bwd:
                out.append(("epi", c.epi))
            if c.bp:
                out.append(("bp", c.bp_bn))
        else:
            out.append(("apply", c.bn))
    for g in groups:
        for i in range(g.n_conv):
            if g.conv[i].pro_bn_relu:
                out.append(("wgrad", g.conv[i].pro))
    return out


@pytest.mark.parametrize("case", CASES, ids=["%s_c%d_m%d_%s" % (c[0], c[1], c[4] * c[3] ** 2, c[5]) for c in CASES])
def test_bn_table_plan(case):
    from realnvp_hip import _lib
    from realnvp_hip import engine as E
    kind, cio, mid, size, B, dtype, _ = case
    eng = _engine(kind, cio, mid, size)
    cpu = torch.device("cpu")
    ws = eng.weights(dtype)
    T = eng._tensors()
    sv = eng.alloc_saved(B, size, size, dtype, cpu, True)
    sc = eng.scratch(B, size, size, dtype, cpu)
    ar = sv["arena"]
    assert E.BN_TABLES is True
    items, groups = eng._bwd_args(T, sv, sc, ws, True)[:2]

    # the table region: one slot per BatchNorm, disjoint, outside the zeroed range
    slots = {}
    for bn, spec in eng.P.bns.items():
        off, nb = ar.slots["t:" + bn]
        assert nb == 4 * _lib.bn_tab_floats(spec.c) and ar.ptr("t:" + bn) % 16 == 0
        slots[ar.ptr("t:" + bn)] = (bn, off, off + nb)
    spans = sorted((o, e) for _, o, e in slots.values())
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
    z0, z1 = ar.range_bytes("in_sums", list(ar.slots)[-1])
    assert all(e <= z0 or o >= z1 for o, e in spans)

    # every backward source reads its own BatchNorm's table (identified by its sums)
    sums_of = {ar.ptr("s:" + bn): bn for bn in eng.P.bns}
    srcs = _bwd_sources(items, groups)
    assert {w for w, _ in srcs} >= {"epi", "apply", "wgrad"}
    for what, s in srcs:
        assert s.sums in sums_of, what
        if what == "wgrad":
            assert not s.tab
            continue
        assert s.tab in slots and slots[s.tab][0] == sums_of[s.sums], (what, sums_of[s.sums])
    # ... all of them are written: the running-statistics update has a row per BatchNorm
    rows = (_lib.BNRunning * sv["bn_n"]).from_buffer_copy(sv["bn_table"].numpy().tobytes())
    assert {r.tab for r in rows} == set(slots)
    for r in rows:
        bn = sums_of[r.sums]
        assert slots[r.tab][0] == bn and r.C == eng.P.bns[bn].c
        assert r.eps == pytest.approx(E.BN_EPS)

    # forward sources: the table is not written yet
    convs = [a for a, _, _ in eng._fwd_args(T, sv, ws, True)]
    assert convs and any(a.pro_bn_relu for a in convs)
    assert all(not a.pro.tab and not a.epi.tab and not a.bp_bn.tab for a in convs)

    # BN_TABLES off: the shard reduction everywhere
    E.BN_TABLES = False
    try:
        it0, gr0 = eng._bwd_args(T, sv, sc, ws, True)[:2]
    finally:
        E.BN_TABLES = True
    assert len(it0) == len(items)
    assert all(not s.tab for _, s in _bwd_sources(it0, gr0))
    # ... and an arena made with it off has no table region and a writer that writes none
    E.BN_TABLES = False
    try:
        sv0 = eng.alloc_saved(B, size, size, dtype, cpu, True)
    finally:
        E.BN_TABLES = True
    assert not any(k.startswith("t:") for k in sv0["arena"].slots)
    rows0 = (_lib.BNRunning * sv0["bn_n"]).from_buffer_copy(sv0["bn_table"].numpy().tobytes())
    assert all(not r.tab for r in rows0)

    # eval plans: running statistics, no table (and no table region)
    sv_e = eng.alloc_saved(B, size, size, dtype, cpu, False)
    assert not any(k.startswith("t:") for k in sv_e["arena"].slots)
    it_e, gr_e = eng._bwd_args(T, sv_e, sc, ws, False)[:2]
    src_e = _bwd_sources(it_e, gr_e)
    assert src_e and all(not s.tab and not s.sums for _, s in src_e)
