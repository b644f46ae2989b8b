"""numpy model of the routing-agreement semantics (include/ringpop_amd.h, rp_ring_route_views*).

A view allows a subset of a base ring's servers; a key's owner under the view is `lookup` on the
ring that holds exactly the view's tokens: filter the base ring's sorted (token, owner) arrays by
allowed[owner], then the first token >= hash, wrapping to the first. tests/test_route_model.py pins
this against the oracle ring after add_remove(remove=masked-out names), so the model does not lean
on the code under test.
"""
import numpy as np

NIL = 0xFFFFFFFF


def view_owners(tok, own, hashes, allowed):
    """uint32[len(hashes)]: owners under one view; allowed: bool per server id."""
    hashes = np.asarray(hashes, dtype=np.uint32)
    keep = np.asarray(allowed, dtype=bool)[own] if len(own) else np.zeros(0, dtype=bool)
    t, o = tok[keep], own[keep]
    if len(t) == 0:
        return np.full(len(hashes), NIL, dtype=np.uint32)
    i = np.searchsorted(t, hashes, "left")
    i[i == len(t)] = 0
    return o[i].astype(np.uint32)


def by_id(rows, col, id_cap):
    """allowed[V][id_cap] by server id from byte / bool rows[V][columns] and a column map
    (None: the identity; NIL: allowed nowhere)."""
    rows = np.asarray(rows) != 0
    if rows.ndim == 1:
        rows = rows[None, :]
    out = np.zeros((rows.shape[0], id_cap), dtype=bool)
    c = np.arange(id_cap, dtype=np.int64) if col is None else np.asarray(col, dtype=np.int64)[:id_cap]
    ok = (c != NIL) & (c < rows.shape[1])
    out[:, np.nonzero(ok)[0]] = rows[:, c[ok]]
    return out


def route(tok, own, hashes, allowed, truth=None, active=None):
    """The five outputs. allowed: bool[V][id]; truth: bool[id] (None: every server of the ring);
    active: bool[V] (None: all)."""
    hashes = np.asarray(hashes, dtype=np.uint32)
    allowed = np.asarray(allowed, dtype=bool)
    nv, n = allowed.shape[0], len(hashes)
    ids = allowed.shape[1]
    if truth is None:
        truth = np.zeros(ids, dtype=bool)
        truth[own] = True
    truth = np.asarray(truth, dtype=bool)
    act = np.ones(nv, dtype=bool) if active is None else np.asarray(active) != 0
    t = view_owners(tok, own, hashes, truth)
    owners = np.full((n, nv), NIL, dtype=np.uint32)
    for v in range(nv):
        owners[:, v] = view_owners(tok, own, hashes, allowed[v])
    diff = owners != t[:, None]
    gone = np.zeros((n, nv), dtype=bool)
    real = owners != NIL
    gone[real] = ~truth[owners[real]]
    return {"wrong": (diff & act[None, :]).sum(axis=0).astype(np.uint64),
            "lost": (gone & act[None, :]).sum(axis=0).astype(np.uint64),
            "key_wrong": (diff & act[None, :]).sum(axis=1).astype(np.uint32),
            "truth_owner": t, "owners": owners}


EDGE_NAMES = ("0", "tok[0]", "tok[0]+1", "tok[M-1]", "tok[M-1]+1", "2^32-1")


def edge_hashes(tok):
    """The six hashes at the ring's ends: 0, the first token and one past it, the last token and
    one past it (the wrap), 2^32 - 1."""
    return np.array([0, int(tok[0]), (int(tok[0]) + 1) & NIL, int(tok[-1]), (int(tok[-1]) + 1) & NIL, NIL],
                    dtype=np.uint32)
