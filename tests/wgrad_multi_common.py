"""Shared by the model-wide weight-gradient tests (rnvp_wgrad_multi_plan /
rnvp_conv2d_wgrad_multi): group construction over host-side conv specs, the
planner call and the decoding of a plan into (conv, slab, co tile, ci tile)."""
import ctypes as C

# tap-shared tile classes (wgrad_tap.hip WtCfg): (co tile, ci tile)
TILE = {0: (64, 64), 1: (128, 128), 2: (32, 32), 3: (64, 64)}
WG_OVERHEAD = 2     # wgrad_tap.hip WT_WG_OVERHEAD: a workgroup's prologue + epilogue, in stages
STAGE = 128         # pixels per stage (WT_SP)


def tile_class(ks, cs_in, cs_dy):
    """wgrad_tap.hip wt_class_base"""
    if ks == 3:
        return 2 if cs_in <= 32 and cs_dy <= 32 else 0
    return 3 if cs_in <= 64 and cs_dy <= 64 else 1


def make_group(B, H, W, convs, ptr, nz=None, nrep=None):
    """A bf16 WgradGroup over convs = [(ks, cin, cout, bias, pro)]; ptr(conv
    index, field) -> address of that conv's buffer ("x", "dy", "ws", "wsb",
    "sums", "gamma", "beta")."""
    from realnvp_hip import _lib
    from realnvp_hip._lib import BNSrc, WgradGroup
    from realnvp_hip.engine import stat_shards
    from realnvp_hip.net import chan_stride, round_up
    L = _lib.lib()
    M = B * H * W
    nz = int(L.wgrad_slabs(M)) if nz is None else nz
    nrep = int(L.wgrad_replicas(nz)) if nrep is None else nrep
    g = WgradGroup()
    g.dtype, g.B, g.H, g.W, g.n_conv = 1, B, H, W, len(convs)
    for i, (ks, cin, cout, bias, pro) in enumerate(convs):
        c = g.conv[i]
        csi, cso = chan_stride(cin), chan_stride(cout)
        c.x, c.cs_in, c.cin, c.ks = ptr(i, "x"), csi, cin, ks
        c.dy, c.cs_dy, c.n = ptr(i, "dy"), cso, cout
        c.ws, c.kp, c.nz, c.nrep = ptr(i, "ws"), round_up(ks * ks * csi, 64), nz, nrep
        c.wsb = ptr(i, "wsb") if bias else None
        if pro:
            c.pro_bn_relu = 1
            c.pro = BNSrc(ptr(i, "sums"), float(M), None, None, ptr(i, "gamma"), ptr(i, "beta"), 1e-5,
                          stat_shards(M))
    return g


def group_array(groups):
    from realnvp_hip._lib import WgradGroup
    arr = (WgradGroup * len(groups))()
    for i, g in enumerate(groups):
        C.memmove(C.addressof(arr[i]), C.addressof(g), C.sizeof(WgradGroup))
    return arr


def plan(groups, cls):
    """(status, WgradMulti, convs, xcd_start list, tasks list of (conv, local))"""
    from realnvp_hip import _lib
    from realnvp_hip._lib import WgradMulti, WgradMultiConv
    L = _lib.lib()
    arr = group_array(groups)
    m = WgradMulti()
    st = L.wgrad_multi_plan(arr, len(groups), cls, None, 0, None, None, 0, C.byref(m))
    if st != 0 or m.n_conv == 0:
        return st, m, None, None, None
    convs = (WgradMultiConv * m.n_conv)()
    xs = (C.c_int * 9)()
    tasks = (C.c_int * (2 * m.n_task))()
    st = L.wgrad_multi_plan(arr, len(groups), cls, convs, m.n_conv, xs, tasks, m.n_task, C.byref(m))
    return st, m, convs, list(xs), [(tasks[2 * i], tasks[2 * i + 1]) for i in range(m.n_task)]


def expected_convs(groups, cls):
    """[(group, conv index in group, nz, co tiles, ci tiles, M, m_per_slab)] of class cls, in table order"""
    out = []
    for gi, g in enumerate(groups):
        M = g.B * g.H * g.W
        for ci in range(g.n_conv):
            c = g.conv[ci]
            if tile_class(c.ks, c.cs_in, c.cs_dy) != cls:
                continue
            tco, tci = TILE[cls]
            stages = -(-M // STAGE)
            mps = -(-stages // c.nz) * STAGE
            out.append((gi, ci, c.nz, -(-c.n // tco), -(-c.cs_in // tci), M, mps))
    return out
