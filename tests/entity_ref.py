"""Shared helpers of the entity-observation tests (tests/test_entities.py, on the emulator and on the device).

The reference for the values is the float64 formula sheet of include/wrsn_hip.h (wrsn_entity_out), evaluated in numpy from wrsn_peek,
the scenario's positions and the specs.  Tolerance, derived: a value is a float64 expression rounded once to float32, and the device may
multiply by a reciprocal where numpy divides (1e-16 relative before the rounding), so the two float32 results are at most one float32
ulp apart: |got - float32(ref)| <= 2^-23 |ref| + 1e-30.  Slots defined as 0 or 1, the level, the asking charger, n_node and all padding
are exact."""
import numpy as np

PATTERN = 0xA5                                                # byte the buffers are filled with before a call
GUARD = 64                                                    # guard bytes on both sides of a buffer (a multiple of 16)
NODE_EXACT = (6, 7)
MC_EXACT = (3, 4, 5, 10, 11)
ENV_EXACT = (4, 5, 6, 7)


def peeks(h):
    """What the reference formulas read, for the whole batch of RawHandle h."""
    return {"nodes": h.nodes(), "mcs": h.mcs(), "env": h.env_info()}


def reference(pk, e, a, sc, mc, N, M):
    """float64 rows (node [N,8], charger [M,12], environment [8]) of environment e for the asking charger a."""
    env = {k: v[e] for k, v in pk["env"].items()}
    xmin, ymin, mtm, ctm = env["xmin"], env["ymin"], env["moving_time_max"], env["charging_time_max"]
    W, H = env["xmax"] - xmin, env["ymax"] - ymin
    a_b2 = mc["alpha"] / mc["beta"] ** 2
    thr, cap = float(sc.node_spec["threshold"]), float(sc.node_spec["capacity"])
    n = sc.n_node
    nd = {k: v[e, :n] for k, v in pk["nodes"].items()}
    node = np.zeros((N, 8))
    node[:n, 0] = (sc.node_xy[:, 0] - xmin) / W
    node[:n, 1] = (sc.node_xy[:, 1] - ymin) / H
    alive = nd["status"] != 0
    E, CS, RR = nd["energy"], nd["cs"], nd["rr"]
    with np.errstate(divide="ignore", invalid="ignore"):
        ef = (E - thr) / (cap - thr)
        node[:n, 2] = np.where(alive, (CS / a_b2) / ef, 0.0)
    node[:n, 3] = np.where(alive, ef, 0.0)
    node[:n, 4] = np.where(alive, CS / a_b2, 0.0)
    node[:n, 5] = np.where(alive, RR / a_b2, 0.0)
    node[:n, 6] = np.where(alive, nd["level"], 0)
    node[:n, 7] = alive
    m = {k: v[e] for k, v in pk["mcs"].items()}
    ch = np.zeros((M, 12))
    for o in range(M):
        lx, ly, c0, c1 = m["loc_x"][o], m["loc_y"][o], m["cur_x"][o], m["cur_y"][o]
        move = 0.0 if o == a else np.sqrt((lx - c0) ** 2 + (ly - m["cur_y"][a]) ** 2) / mc["velocity"] / mtm   # WRSN.py:184, mixed index
        ch[o] = [(lx - xmin) / W, (ly - ymin) / H, m["energy"][o] / mc["capacity"], float(o == a), float(m["status"][o] != 0),
                 float(m["type_charging"][o] != 0), (c0 - xmin) / W, (c1 - ymin) / H, m["cur_t"][o] / ctm, move, 0.0, 0.0]
    t = min(W, H)
    envr = np.array([mc["charging_range"] / W, mc["charging_range"] / H, 0.5 * t / W, 0.5 * t / H, float(a), float(n), 0.0, 0.0])
    return node, ch, envr


def _check(got, ref, exact, tag):
    g = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    r32 = ref.astype(np.float32).astype(np.float64)
    ok = np.where(exact, g == ref, np.abs(g - r32) <= 2.0 ** -23 * np.abs(ref) + 1e-30)
    assert ok.all(), (tag, np.argwhere(~ok)[:5].tolist(), g[~ok][:5], ref[~ok][:5])


def check_rows(got, ref, n_node, tag=""):
    """got / ref: (node, charger, environment) rows of one environment with n_node nodes of its own."""
    node, ch, envr = ref
    ex = np.zeros(node.shape, dtype=bool)
    ex[:, list(NODE_EXACT)] = True
    ex[n_node:] = True                                        # padding rows
    ex[:n_node][node[:n_node, 7] == 0, 2:] = True              # a dead node: zeros
    _check(got[0], node, ex, tag + " node")
    ex = np.zeros(ch.shape, dtype=bool); ex[:, list(MC_EXACT)] = True
    ex[:, 9] = ch[:, 3] == 1                                  # 0 for the asking charger
    _check(got[1], ch, ex, tag + " charger")
    ex = np.zeros(envr.shape, dtype=bool); ex[list(ENV_EXACT)] = True
    _check(got[2], envr, ex, tag + " env")


def splat(node, ch, envr, G):
    """The four maps of get_state (WRSN.py:130-186) from entity rows, with the reference's func."""
    def func(x, h):
        return np.exp(x ** 2 / (-2 * h ** 2))
    c = np.arange(G) / G + 0.5 / G
    maps = np.zeros((4, G, G))
    hX, hY, sX, sY = envr[:4]
    for r in node[node[:, 7] == 1]:
        maps[0] += r[2] * np.outer(func(c - r[0], hX), func(c - r[1], hY))
    for r in ch:
        if r[3] == 1:
            maps[1] += r[2] * np.outer(func(c - r[0], sX), func(c - r[1], sY))
        elif r[5] == 1:
            maps[2] += r[8] * np.outer(func(c - r[6], hX), func(c - r[7], hY))
        else:
            maps[3] += r[9] * np.outer(func(c - r[6], hX), func(c - r[7], hY))
    return maps


class EntBuf:
    """The three entity buffers with GUARD bytes on both sides, in numpy (the emulator's device memory) or, with `device`, in torch
    tensors on that device.  `snap()` gives host copies {name: uint8 array with the guards}; the checks below work on those."""

    def __init__(self, B, N, M, device=None):
        self.B, self.N, self.M = B, N, M
        self.shapes = {"node": (B, N, 8), "mc": (B, M, 12), "env": (B, 8)}
        self.raw = {}
        for k, sh in self.shapes.items():
            n = int(np.prod(sh)) * 4 + 2 * GUARD
            if device is None:
                buf = np.empty(n + 16, dtype=np.uint8)
                off = (-buf.ctypes.data) % 16
            else:
                import torch
                buf = torch.empty(n + 16, dtype=torch.uint8, device=device)
                off = (-buf.data_ptr()) % 16
            self.raw[k] = buf[off:off + n]
        self.fill()

    def fill(self):
        for r in self.raw.values():
            r[:] = PATTERN

    def ptr(self, k):
        r = self.raw[k]
        return (r.ctypes.data if isinstance(r, np.ndarray) else r.data_ptr()) + GUARD

    def ptrs(self):
        return self.ptr("node"), self.ptr("mc"), self.ptr("env")

    def snap(self):
        return {k: (r.copy() if isinstance(r, np.ndarray) else r.cpu().numpy()) for k, r in self.raw.items()}

    def rows(self, snap, e):
        """(node, charger, environment) float32 rows of environment e."""
        return tuple(snap[k][GUARD:-GUARD].view(np.float32).reshape(self.shapes[k])[e] for k in ("node", "mc", "env"))

    def row_bytes(self, snap, e):
        return np.concatenate([snap[k][GUARD:-GUARD].reshape(self.B, -1)[e] for k in ("node", "mc", "env")])

    def guards_intact(self, snap):
        return all((s[:GUARD] == PATTERN).all() and (s[-GUARD:] == PATTERN).all() for s in snap.values())

    def untouched(self, snap, e):
        return bool((self.row_bytes(snap, e) == PATTERN).all())

    def full(self, snap, e):
        """No 4-byte slot of row e still holds the pattern."""
        return bool((self.row_bytes(snap, e).view(np.uint32) != PATTERN * 0x01010101).all())


def check_extent(buf, snap, rendered, tag=""):
    """Guards intact; rows of `rendered` written in every slot; every other row byte for byte the pattern."""
    assert buf.guards_intact(snap), (tag, "guard bytes")
    for e in range(buf.B):
        if e in rendered:
            assert buf.full(snap, e), (tag, "row %d holds pattern bytes" % e)
        else:
            assert buf.untouched(snap, e), (tag, "row %d was touched" % e)
