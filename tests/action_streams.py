"""TEST INFRASTRUCTURE -- policy-shaped action streams for the parity tests (tests/test_action_streams.py).

The random policy of tests/parity.py (`rng.rand(B, 3)`) spreads the chargers over the field.  What the shipped policies do is different:
they send several chargers to the same critical node, they sit on the clip edges, they ask for charging times of exactly zero, they repeat
themselves.  A stream here is a function of what the oracle and the device expose identically at a request -- the asking charger, the
oracle's node and charger state, the frame of the network, a seeded RandomState -- and returns the NORMALISED action (WRSN.py:293-299:
clipped to [0, 1], then `translate`d, WRSN.py:95-98).  It is computed once per request and handed to both sides.

    make(name, seed) -> stream;  stream(req) -> np.array([x, y, charge]);  req: a Request

A stream keeps its own memory (the fixed point of `same_spot`, the action `repeat` repeats) and its own RandomState, so a stream per
environment makes a batch reproducible from the seeds."""
import collections

import numpy as np

# agent: the asking charger; nodes / mcs: OracleWRSN.nodes() / .mcs() at the request; frame: (xmin, xmax, ymin, ymax) of env_info();
# node_xy: [N, 2]; k: requests this environment has had so far
Request = collections.namedtuple("Request", "agent nodes mcs frame node_xy k")

NAMES = ("converge", "same_spot", "same_spot_on_node", "zero_charge", "stay", "clip_edges", "repeat", "mixed")
JITTER = 0.01                                                # converge: +- this much of the frame per axis
SHORT_CHARGE = (0.02, 0.15)                                  # of charging_time_max (WRSN.py:51)
REPEAT_N = 4


def down(frame, xy):
    """WRSN.down_mapping (WRSN.py:86-88)."""
    return np.array([(xy[0] - frame[0]) / (frame[1] - frame[0]), (xy[1] - frame[2]) / (frame[3] - frame[2])])


def up(frame, a):
    """The position part of WRSN.translate (WRSN.py:95-97), same operations in the same order."""
    return np.array([a[0] * (frame[1] - frame[0]) + frame[0], a[1] * (frame[3] - frame[2]) + frame[2]])


def exact_down(frame, xy):
    """A normalised position that `translate` maps back onto `xy` bit for bit, and whether one was found: the quotient of down_mapping,
    or one of its neighbours a few ulp away (the round trip is a division, a multiplication and an addition: it misses by an ulp or two
    about as often as it hits)."""
    a = down(frame, xy); hit = [False, False]
    for ax in range(2):
        lo, w = frame[2 * ax], frame[2 * ax + 1] - frame[2 * ax]
        cand = [a[ax]]
        for s in (np.inf, -np.inf):
            c = a[ax]
            for _ in range(4):
                c = np.nextafter(c, s); cand.append(c)
        for c in cand:
            if 0.0 <= c <= 1.0 and c * w + lo == xy[ax]:
                a[ax] = c; hit[ax] = True
                break
    return a, all(hit)


def _short(rng):
    return rng.uniform(*SHORT_CHARGE)


def _weakest(req):
    """The alive node of least energy (the first of them in id order)."""
    alive = req.nodes["status"] == 1
    e = np.where(alive, req.nodes["energy"], np.inf)
    return int(np.argmin(e))


class Stream:
    """One stream: `name`, its RandomState, its memory; `exact_stays` counts the `stay` actions whose destination is the charger's
    location bit for bit (moving_time == 0, MobileCharger.py:83-87)."""

    def __init__(self, name, seed):
        assert name in NAMES, name
        self.name, self.rng, self.mem, self.exact_stays, self.used = name, np.random.RandomState(seed), {}, 0, collections.Counter()

    def __call__(self, req):
        name = self.name
        if name == "mixed":
            if not self.mem.get("order"):                    # every stream but `mixed` itself, each once per round, in a seeded order
                self.mem["order"] = list(self.rng.permutation(len(NAMES) - 1))
            name = NAMES[self.mem["order"].pop()]
        self.used[name] += 1
        a = getattr(self, "_" + name)(req)
        return np.asarray(a, dtype=np.float64)

    # every charger is sent to the node that is about to die: charging discs overlap, two chargers hold the same node
    def _converge(self, req):
        i = _weakest(req)
        p = down(req.frame, req.node_xy[i]) + self.rng.uniform(-JITTER, JITTER, 2)
        return [p[0], p[1], _short(self.rng)]

    # one fixed point for every charger and the whole episode
    def _same_spot(self, req):
        if "spot" not in self.mem:                           # a few metres off a node, so that the discs hold something
            i = self.rng.randint(len(req.node_xy))
            self.mem["spot"] = down(req.frame, req.node_xy[i] + self.rng.uniform(-8.0, 8.0, 2))
        return [self.mem["spot"][0], self.mem["spot"][1], _short(self.rng)]

    # ... the point being a node's position, as exactly as the normalisation allows: distance 0 in the charging rate (Node.py:137)
    def _same_spot_on_node(self, req):
        if "node" not in self.mem:
            self.mem["node"] = _weakest(req)
        p, _ = exact_down(req.frame, req.node_xy[self.mem["node"]])
        return [p[0], p[1], _short(self.rng)]

    # charging time exactly 0 on three requests of four (`tmp == 0`, MobileCharger.py:60), the destination one of three fixed points (a
    # collapsed policy): a charger sent where it already stands moves for the few ulps by which its summed-up position misses the
    # point, and is back at the same instant
    def _zero_charge(self, req):
        if "spots" not in self.mem:
            self.mem["spots"] = self.rng.uniform(0.1, 0.9, (3, 2))
        p = self.mem["spots"][self.rng.randint(3)]
        c = _short(self.rng) if self.rng.randint(4) == 0 else 0.0
        return [p[0], p[1], c]

    # destination = where the charger is: moving_time == 0 (MobileCharger.py:83-87); charge zero or short
    def _stay(self, req):
        loc = np.array([req.mcs["loc_x"][req.agent], req.mcs["loc_y"][req.agent]])
        p, hit = exact_down(req.frame, loc)
        self.exact_stays += int(hit)
        c = _short(self.rng) if self.rng.randint(3) == 0 else 0.0
        return [p[0], p[1], c]

    # components outside and on the edges of [0, 1]: both sides clip (WRSN.py:299); the corners of the frame, charging time 0 or the maximum
    # (inside `mixed` the charge component stays on the lower edge: a charging time of charging_time_max ends the episode within a
    # dozen requests, before the budgeted and time-sliced launches have seen much)
    def _clip_edges(self, req):
        a = self.rng.choice([-0.5, 0.0, 1.0, 1.5], 3)
        if self.name == "mixed":
            a[2] = self.rng.choice([-0.5, 0.0])
        return a

    # one action, verbatim, REPEAT_N times per charger
    def _repeat(self, req):
        a, n = self.mem.get(("rep", req.agent), (None, 0))
        if n == 0:
            p = self.rng.rand(2)
            a, n = np.array([p[0], p[1], _short(self.rng)]), REPEAT_N
        self.mem[("rep", req.agent)] = (a, n - 1)
        return a.copy()


def make(name, seed):
    return Stream(name, seed)


def shared_nodes(req, node_status, charging_range):
    """Path coverage of `converge` / `same_spot`: the alive nodes inside the charging range of at least two chargers that are at
    action type `charging` with connected nodes (WRSN.py:116-126, MobileCharger.py:55-58), from the oracle's charger positions."""
    m = req.mcs
    on = [k for k in range(len(m["loc_x"])) if m["type_charging"][k] == 1 and m["n_conn"][k] > 0 and m["status"][k] != 0]
    if len(on) < 2:
        return np.zeros(0, dtype=int)
    cover = np.zeros(len(req.node_xy), dtype=int)
    for k in on:
        d = np.sqrt(((req.node_xy - np.array([m["loc_x"][k], m["loc_y"][k]])) ** 2).sum(1))
        cover += d <= charging_range
    return np.nonzero((cover >= 2) & (node_status == 1))[0]
