"""The flow program (realnvp_hip/program.py) without a GPU: the schedule and
its derived inverse against literals typed from the reference's f and g
(flow_realnvp.py:252-327, 196-249), and the buffer wiring of FlowProgram
against the oracle's permutations (couplings as the identity)."""
import pytest
import torch

import realnvp_oracle as O

C3, C4 = ["coupling"] * 3, ["coupling"] * 4
R3, R4 = ["reverse"] * 3, ["reverse"] * 4


def f_literal(n_scales):
    """reference f: per scale 3 checkerboard couplings, squeeze, 3 channelwise
    couplings, undo, factor_out; 4 couplings at the last scale; the restores"""
    return (C3 + ["squeeze"] + C3 + ["undo", "factor_out"]) * (n_scales - 1) + C4 + ["restore"] * (n_scales - 1)


def g_literal(n_scales):
    """reference g: the factor_outs, the last scale's couplings reversed, then
    per scale restore, squeeze, reversed channelwise, undo, reversed checkerboard"""
    return ["factor_out"] * (n_scales - 1) + R4 + (["restore", "squeeze"] + R3 + ["undo"] + R3) * (n_scales - 1)


def make_model(n_scales, size=None):
    import flow_realnvp
    import utils
    size = size or (1 << n_scales)
    return flow_realnvp.RealNVP(3, size, None, utils.Hyperparameters(4, 1, True, True, True, True), n_scales=n_scales)


def test_literals_spelled_out_at_three_scales():
    """the two generators above, against the sequences typed out in full"""
    assert f_literal(3) == [
        "coupling", "coupling", "coupling", "squeeze", "coupling", "coupling", "coupling", "undo", "factor_out",
        "coupling", "coupling", "coupling", "squeeze", "coupling", "coupling", "coupling", "undo", "factor_out",
        "coupling", "coupling", "coupling", "coupling", "restore", "restore"]
    assert g_literal(3) == [
        "factor_out", "factor_out", "reverse", "reverse", "reverse", "reverse",
        "restore", "squeeze", "reverse", "reverse", "reverse", "undo", "reverse", "reverse", "reverse",
        "restore", "squeeze", "reverse", "reverse", "reverse", "undo", "reverse", "reverse", "reverse"]


@pytest.mark.parametrize("n_scales", [2, 3, 5, 6])
def test_schedule_and_derived_inverse_equal_the_reference_literals(n_scales):
    from realnvp_hip.program import flow_schedule, inverse_schedule
    model = make_model(n_scales)
    ops = flow_schedule(model)
    assert [k for k, _ in ops] == f_literal(n_scales)
    mods = [m for _, m in ops if m is not None]
    assert len(mods) == 6 * (n_scales - 1) + 4
    assert all(a is b for a, b in zip(mods, model.couplings()))
    assert all((m is None) == (k != "coupling") for k, m in ops)
    inv = inverse_schedule(ops)
    assert [k for k, _ in inv] == g_literal(n_scales)
    assert all(a is b for a, b in zip([m for _, m in inv if m is not None], reversed(mods)))
    assert inverse_schedule(inv) == ops


def _program(n_scales=3, B=2, size=16):
    from realnvp_hip.program import FlowProgram
    model = make_model(n_scales, size)
    # the coupling allocation (engine, saved activations, gradient block) stubbed out
    return model, FlowProgram(model, B, "cpu", "fp32", False, alloc=lambda mod, x: (None, None, None))


def _interpret(st):
    """a stage with the oracle's permutations; a coupling is the identity"""
    if st.kind == "coupling":
        st.z.copy_(st.x)
    elif st.kind == "reverse":
        st.x.copy_(st.z)
    elif st.kind == "squeeze":
        st.b.copy_(O.squeeze(st.a))
    elif st.kind == "undo":
        st.b.copy_(O.undo_squeeze(st.a))
    elif st.kind == "factor_out":
        on, off = O.factor_out(st.a)
        st.on.copy_(on)
        st.off.copy_(off)
    else:
        assert st.kind == "restore"
        st.full.copy_(O.restore(st.on, st.off))


def test_program_wiring_against_the_oracle():
    from realnvp_hip.program import inverse_perm
    _, prog = _program()
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    # the same chain written straight with the oracle functions (n_scales = 3)
    z = O.undo_squeeze(O.squeeze(x))
    z, off1 = O.factor_out(z)
    z = O.undo_squeeze(O.squeeze(z))
    z, off2 = O.factor_out(z)
    ref = O.restore(O.restore(z, off2), off1)
    for t in [prog.x] + [t for st in prog.stages for t in st if isinstance(t, torch.Tensor)]:
        t.fill_(float("nan"))
    prog.x.copy_(x)
    for st in prog.stages:
        _interpret(st)
    assert torch.equal(prog.z, ref)
    # the derived inverse over the same buffers returns the input bit for bit
    prog.x.fill_(float("nan"))
    for st in reversed(prog.stages):
        _interpret(st._replace(kind="reverse") if st.kind == "coupling" else inverse_perm(st))
    assert torch.equal(prog.x, x)


def test_every_output_is_the_next_consumers_input():
    """by identity: a mis-wired off buffer has the right shape"""
    _, prog = _program()
    reads = {"coupling": ("x",), "squeeze": ("a",), "undo": ("a",), "factor_out": ("a",), "restore": ("on", "off")}
    writes = {"coupling": ("z",), "squeeze": ("b",), "undo": ("b",), "factor_out": ("on", "off"), "restore": ("full",)}
    cur, offs, seen = prog.x, [], {id(prog.x)}
    for st in prog.stages:
        ins = [getattr(st, f) for f in reads[st.kind]]
        outs = [getattr(st, f) for f in writes[st.kind]]
        assert ins[0] is cur, st.kind
        if st.kind == "restore":
            assert ins[1] is offs.pop()        # the latest factored-out half, each exactly once
        for t in outs:
            assert id(t) not in seen           # every output is a buffer of its own
            seen.add(id(t))
        if st.kind == "factor_out":
            offs.append(st.off)
        cur = outs[0]
    assert cur is prog.z and not offs
    # one output per coupling, sq / un / on / off per scale, one full per restore, and the input
    n_scales, n_coupling = 3, 16
    assert len(seen) == 1 + n_coupling + 4 * (n_scales - 1) + (n_scales - 1)


def test_stage_records_are_tuples_in_the_trainer_order():
    model, prog = _program()
    st = prog.couplings[0]
    kind, mod, eng, x, z, sv, block = st
    assert kind == "coupling" and mod is next(model.couplings()) and x is prog.x and z is st.z
    assert (eng, sv, block) == (None, None, None) and (st.eng, st.saved, st.block) == (None, None, None)
    assert isinstance(st, tuple) and st[0] == "coupling" and st[3] is x
    by_kind = {s.kind: s for s in prog.stages}
    _, a, b = by_kind["squeeze"]
    assert tuple(b.shape) == (2, 4 * a.shape[1], a.shape[2] // 2, a.shape[3] // 2)
    _, a, b = by_kind["undo"]
    assert tuple(a.shape) == (2, 4 * b.shape[1], b.shape[2] // 2, b.shape[3] // 2)
    _, a, on, off = by_kind["factor_out"]
    assert on.shape == off.shape == (2, 2 * a.shape[1], a.shape[2] // 2, a.shape[3] // 2)
    _, on, off, full = by_kind["restore"]
    assert on.shape == off.shape == (2, 2 * full.shape[1], full.shape[2] // 2, full.shape[3] // 2)
