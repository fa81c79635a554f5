"""rnvp_wgrad_multi_plan (host only, no GPU): the block -> task map of the
model-wide weight-gradient launch.

For a deep-coupling-like list at B = 64 (4x4 / 8x8 / 16x16, dims 512 / 256 /
128, two couplings each) and for a mixed list of three small shapes, per tile
class:
  * every (conv, slab, co tile, ci tile) appears exactly once, surplus blocks
    (the grid is 8 x the longest XCD list) map to no task, and the tiles of a
    (conv, slab) are adjacent on one XCD;
  * the largest XCD cost is at most the mean plus the heaviest single run
    (the greedy longest-first bound: when the most loaded XCD received its
    last run it was the least loaded, i.e. at most at the mean), every XCD's
    list is ordered by descending tile cost and the reported costs are the
    sums of stages + overhead over the XCD's tiles;
  * a second call returns the identical plan;
  * a conv with nrep < nz (atomic accumulation) is refused, as is a group
    from 65,536 pixels up (per-class launches of its own)."""
import pytest

from wgrad_multi_common import STAGE, WG_OVERHEAD, expected_convs, make_group, plan


def _ptr(base):
    # fake 256-byte aligned addresses: the planner never dereferences them
    order = ["x", "dy", "ws", "wsb", "sums", "gamma", "beta"]
    return lambda i, f: base + (i * 8 + order.index(f) + 1) * 256


def _net(cin, d, cout):
    """an s/t net's convs, (ks, cin, cout, bias, pro): in conv, two bottleneck
    blocks with their skips, out conv"""
    convs = [(3, cin, d, True, False), (1, d, d, True, False)]
    for _ in range(2):
        convs += [(1, d, d, False, True), (3, d, d, False, True), (1, d, d, True, True), (1, d, d, True, False)]
    convs.append((1, d, cout, True, True))
    return convs


def deep_list():
    gs = []
    for k, (hw, d, cin) in enumerate([(16, 128, 25), (16, 128, 25), (8, 256, 49), (8, 256, 49), (4, 512, 97),
                                      (4, 512, 97)]):
        gs.append(make_group(64, hw, hw, _net(cin, d, 2 * (cin - 1)), _ptr((k + 1) << 20)))
    return gs


def mixed_list():
    return [
        make_group(2, 4, 4, [(3, 128, 128, False, False), (1, 160, 96, True, False)], _ptr(1 << 20)),
        make_group(2, 8, 8, [(3, 97, 128, False, True), (1, 128, 128, False, False)], _ptr(2 << 20)),
        make_group(2, 16, 16, [(3, 128, 128, True, False), (1, 160, 96, False, True), (1, 24, 40, True, False),
                               (3, 24, 24, False, False)], _ptr(3 << 20), nz=4, nrep=4),
    ]


LISTS = {"deep_b64": deep_list, "mixed3": mixed_list}


@pytest.mark.parametrize("name", sorted(LISTS))
def test_plan_covers_every_tile_once(name):
    groups = LISTS[name]()
    present = 0
    for cls in range(4):
        st, m, convs, xs, tasks = plan(groups, cls)
        assert st == 0
        exp = expected_convs(groups, cls)
        assert m.n_conv == len(exp)
        if not exp:
            assert m.n_task == 0 and m.grid == 0
            continue
        present += 1
        assert m.cls == cls
        # the table carries each conv's own shape and tiling
        for e, (gi, ci, nz, tco, tci, M, mps) in zip(convs, exp):
            g = groups[gi]
            c = g.conv[ci]
            assert (e.B, e.H, e.W, e.cls) == (g.B, g.H, g.W, cls)
            assert (e.x, e.dy, e.ws, e.wsb) == (c.x, c.dy, c.ws, c.wsb)
            assert (e.cs_in, e.cin, e.cs_dy, e.n, e.kp, e.nz, e.nrep) == (c.cs_in, c.cin, c.cs_dy, c.n, c.kp, nz, nz)
            assert (e.tco, e.tci, e.m_per_slab, e.pro_bn_relu) == (tco, tci, mps, c.pro_bn_relu)
        want = {(k, z, a, b) for k, (_, _, nz, tco, tci, _, _) in enumerate(exp)
                for z in range(nz) for a in range(tco) for b in range(tci)}
        assert xs[0] == 0 and xs[8] == m.n_task == len(want) and all(xs[i] <= xs[i + 1] for i in range(8))
        lens = [xs[i + 1] - xs[i] for i in range(8)]
        assert m.grid == 8 * max(lens)
        # the kernel's map: block b -> XCD b % 8, entry b // 8 of its list
        seen, where, cost, idle = set(), {}, [0] * 8, 0
        tcost = [[] for _ in range(8)]
        for b in range(m.grid):
            x, i = b % 8, b // 8
            if i >= lens[x]:
                idle += 1
                continue
            k, local = tasks[xs[x] + i]
            assert 0 <= k < len(exp)
            _, _, nz, tco, tci, M, mps = exp[k]
            z, rr = divmod(local, tco * tci)
            a, bb = divmod(rr, tci)
            assert 0 <= z < nz
            assert (k, z, a, bb) not in seen
            seen.add((k, z, a, bb))
            where.setdefault((k, z), []).append((x, i))
            stages = -(-(min((z + 1) * mps, M) - z * mps) // STAGE)
            assert stages >= 1
            cost[x] += stages + WG_OVERHEAD
            tcost[x].append(stages + WG_OVERHEAD)
        assert seen == want
        assert idle == m.grid - m.n_task
        # a (conv, slab)'s tiles: one XCD, adjacent
        runs = []
        for (k, z), pos in where.items():
            assert len({x for x, _ in pos}) == 1, (k, z)
            idx = sorted(i for _, i in pos)
            assert idx == list(range(idx[0], idx[0] + len(idx))), (k, z)
            assert len(idx) == exp[k][3] * exp[k][4]
            runs.append(sum(1 for _ in idx) * tcost[pos[0][0]][idx[0]])
        assert list(m.xcd_cost) == cost
        assert max(cost) <= sum(cost) / 8.0 + max(runs)
        for x in range(8):
            assert tcost[x] == sorted(tcost[x], reverse=True)
        # deterministic
        st2, m2, convs2, xs2, tasks2 = plan(groups, cls)
        assert st2 == 0 and xs2 == xs and tasks2 == tasks and bytes(convs2) == bytes(convs)
        assert bytes(m2)[:-24] == bytes(m)[:-24]
    assert present >= 2


def test_plan_refuses_atomic_and_wide_groups():
    from realnvp_hip import _lib
    L = _lib.lib()
    ok = make_group(64, 16, 16, [(3, 128, 128, True, True)], _ptr(1 << 20))
    assert plan([ok], 0)[0] == 0
    # 20,480 pixels: 10 slabs on 8 replicas -> atomics
    M = 80 * 16 * 16
    assert int(L.wgrad_replicas(int(L.wgrad_slabs(M)))) < int(L.wgrad_slabs(M))
    atomic = make_group(80, 16, 16, [(3, 128, 128, True, True)], _ptr(2 << 20))
    for cls in range(4):
        assert plan([atomic], cls)[0] == -2
        assert plan([ok, atomic], cls)[0] == -2
    same_px = make_group(80, 16, 16, [(3, 128, 128, True, True)], _ptr(2 << 20), nz=8, nrep=8)
    assert plan([same_px], 0)[0] == 0
    wide = make_group(64, 32, 32, [(3, 64, 64, True, True)], _ptr(3 << 20), nz=8, nrep=8)
    assert plan([wide], 0)[0] == -2
    fp32 = make_group(64, 16, 16, [(3, 128, 128, True, True)], _ptr(4 << 20))
    fp32.dtype = 0
    assert plan([fp32], 0)[0] == -2
