"""The numpy model of the simulator's census (rp_sim_census) over stacked views,
written straight from the table of outputs.

st, inc, ring: [NL, N] arrays, row lv the view of local node lv (status 0..3 = alive, suspect,
faulty, leave; incarnation; in its ring). observe: bool[NL], the rows that count. ref: int64[N]
or None (then the census' own max_inc)."""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min


def census(st, inc, ring, observe, ref=None):
    st = np.asarray(st, dtype=np.uint8)
    inc = np.asarray(inc, dtype=np.int64)
    ring = np.asarray(ring, dtype=bool)
    nl, n = st.shape
    obs = np.asarray(observe, dtype=bool)
    assert obs.shape == (nl,) and inc.shape == st.shape == ring.shape
    s, x, g = st[obs], inc[obs], ring[obs]
    n_obs = int(obs.sum())
    status = np.stack([(s == k).sum(axis=0) for k in range(4)], axis=1).astype(np.uint32)
    max_inc = x.max(axis=0) if n_obs else np.full(n, INT64_MIN, dtype=np.int64)
    r = max_inc if ref is None else np.asarray(ref, dtype=np.int64)
    behind = np.zeros(nl, dtype=np.uint32)
    behind[obs] = (x < r[None, :]).sum(axis=1)
    return {"observers": n_obs, "status": status, "in_ring": g.sum(axis=0).astype(np.uint32),
            "max_inc": max_inc.astype(np.int64), "at_max": (x == r[None, :]).sum(axis=0).astype(np.uint32),
            "behind": behind}


def same(got, want):
    """None when the two censuses agree field by field (values, dtypes, shapes); else the field."""
    for k in ("status", "in_ring", "max_inc", "at_max", "behind"):
        if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]):
            return k
    return None if int(got["observers"]) == int(want["observers"]) else "observers"
