"""numpy model of routing agreement over the hash space (include/ringpop_amd.h,
rp_ring_route_share*): on how many of the 2^32 hash values every view disagrees with the truth.

The owners are those of tests/routing_model.py at hashes = tok, and nothing else: owner(v, h) is
constant on the interval of every token position, and a hash equal to a token sits at that token's
position, so `routing_model.route(tok, own, tok, ...)` weighted by the interval lengths is the
answer. tests/test_route_share_model.py checks the piecewise constancy this leans on.

`scan` restates the same numbers the way the kernels compute them (the generate / propagate
recurrence, composed per chunk, with the cyclic wrap value), so the algebra is pinned on the CPU.
"""
import numpy as np

import routing_model as rm

NIL = rm.NIL


def lengths(tok):
    """uint64[M]: how many hashes have their lookup position at each token (they sum to 2^32)."""
    t = np.asarray(tok, dtype=np.uint32).astype(np.int64)
    if len(t) == 0:
        return np.zeros(0, dtype=np.uint64)
    return np.diff(t, prepend=t[-1] - (1 << 32)).astype(np.uint64)


def share(tok, own, allowed, truth=None, active=None):
    """{"wrong", "lost": uint64[V], "pos_wrong": uint32[M]}; arguments as routing_model.route."""
    allowed = np.asarray(allowed, dtype=bool)
    r = rm.route(tok, own, tok, allowed, truth, active)
    ln = lengths(tok)
    nv = allowed.shape[0]
    act = np.ones(nv, dtype=bool) if active is None else np.asarray(active) != 0
    if truth is None:
        truth = np.zeros(allowed.shape[1], dtype=bool)
        truth[own] = True
    truth = np.asarray(truth, dtype=bool)
    owners = r["owners"]  # [M, V]
    diff = (owners != r["truth_owner"][:, None]) & act[None, :]
    real = owners != NIL
    gone = np.zeros_like(diff)
    gone[real] = ~truth[owners[real]]
    gone &= act[None, :]
    return {"wrong": (diff * ln[:, None]).sum(axis=0, dtype=np.uint64),
            "lost": (gone * ln[:, None]).sum(axis=0, dtype=np.uint64),
            "pos_wrong": r["key_wrong"]}


def disputed(tok, pos_wrong):
    """The hash values on which at least one counted view disagrees."""
    return int(lengths(tok)[np.asarray(pos_wrong) > 0].sum())


def scan(tok, own, allowed, truth=None, active=None, chunk=64):
    """The same three outputs by the (g, p) recurrences, chunked as the kernels chunk them:
         W_k = (P_k ^ T_k)  | (~P_k & ~T_k & W_{k+1})
         L_k = (P_k & ~T_k) | (~P_k        & L_{k+1})        (cyclic in k)
    pass 1 composes every chunk's (g, p); pass 2 composes the chunks from the last to the first,
    takes the whole ring's generate bit G as the value entering position M - 1 from position 0,
    and hands every chunk the bits entering its last position; pass 3 walks every chunk down."""
    allowed = np.asarray(allowed, dtype=bool)
    nv, m = allowed.shape[0], len(tok)
    act = np.ones(nv, dtype=bool) if active is None else np.asarray(active) != 0
    if truth is None:
        truth = np.zeros(allowed.shape[1], dtype=bool)
        truth[own] = True
    truth = np.asarray(truth, dtype=bool)
    out = {"wrong": np.zeros(nv, dtype=np.uint64), "lost": np.zeros(nv, dtype=np.uint64),
           "pos_wrong": np.zeros(m, dtype=np.uint32)}
    if m == 0:
        return out
    ln = lengths(tok)
    P = allowed[:, own].T  # [M, V]
    T = truth[own][:, None]  # [M, 1]
    g = {"w": P ^ T, "l": P & ~T}
    p = {"w": ~P & ~T, "l": ~P}
    bounds = [(lo, min(lo + chunk, m)) for lo in range(0, m, chunk)]
    enter = {}
    for x in ("w", "l"):
        # pass 1: a chunk's aggregate, composed upwards: (G, Pp) o (g_k, p_k) = (G | Pp & g_k, Pp & p_k)
        agg = []
        for lo, hi in bounds:
            G, Pp = np.zeros(nv, dtype=bool), np.ones(nv, dtype=bool)
            for k in range(lo, hi):
                G, Pp = G | (Pp & g[x][k]), Pp & p[x][k]
            agg.append((G, Pp))
        # pass 2: the whole ring's generate bit, then the carries
        tot = np.zeros(nv, dtype=bool)
        for G, Pp in reversed(agg):
            tot = G | (Pp & tot)
        carry, cur = [None] * len(agg), tot
        for c in range(len(agg) - 1, -1, -1):
            carry[c] = cur
            cur = agg[c][0] | (agg[c][1] & cur)
        assert np.array_equal(cur, tot)  # once round the ring: the value at position 0 again
        enter[x] = carry
    # pass 3
    for c, (lo, hi) in enumerate(bounds):
        w, l = enter["w"][c].copy(), enter["l"][c].copy()
        for k in range(hi - 1, lo - 1, -1):
            w = g["w"][k] | (p["w"][k] & w)
            l = g["l"][k] | (p["l"][k] & l)
            out["wrong"][w & act] += ln[k]
            out["lost"][l & act] += ln[k]
            out["pos_wrong"][k] = int((w & act).sum())
    return out
