"""The key forms a pass over a key stream takes (moved keys, hand-off), for the GPU tests of those
passes: the same n 36-byte UUID keys as

    aligned    36-byte stride at a 16-byte aligned base (the staged tiles' 16-B loads)
    lead4      36-byte stride at a base that is 4-byte but not 16-byte aligned (dword staging)
    lead1      36-byte stride at an odd base (the per-thread byte fetch)
    offsets    mixed lengths of 1..36 bytes behind uint64 offsets
    stride20   the first 20 bytes of every key at stride 20
    hashes     caller hashes (a hashFunc's), which only the host entry points take

host_side() is what the oracle looks up for a form, device_side() what a *_dev call (or, for
`hashes`, a *_hashes call) is given.
"""
import functools

import numpy as np

NIL = 0xFFFFFFFF
FORMS = ("aligned", "lead4", "lead1", "offsets", "stride20", "hashes")
_LEAD = {"aligned": 0, "lead4": 4, "lead1": 1}


@functools.lru_cache(maxsize=None)
def _fixed(n):
    import pyoracle
    k = pyoracle.uuid_keys(42, 0, n)
    k.setflags(write=False)
    return k


def _var(n):
    fixed = _fixed(n)
    return [bytes(fixed[i, :1 + (i * 5) % 36]) for i in range(n)]  # mixed lengths, 1..36 bytes


@functools.lru_cache(maxsize=None)
def host_side(form, n):
    """("keys", uint8[n, L]) or ("hashes", uint32[n]): what the oracle looks up. Read-only."""
    import pyoracle
    if form in _LEAD:
        return "keys", _fixed(n)
    if form == "stride20":
        out = np.ascontiguousarray(_fixed(n)[:, :20])
    elif form == "offsets":
        out = np.array([pyoracle.hash32(k) for k in _var(n)], dtype=np.uint32)
    else:
        out = np.random.default_rng(36).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    out.setflags(write=False)
    return ("keys" if form == "stride20" else "hashes"), out


def oracle_rows(o, form, n, nrep):
    """The oracle ring o's lookupN rows [n, max(nrep, 1)] of the form's keys, in the oracle's ids."""
    kind, data = host_side(form, n)
    if kind == "keys":
        return o.lookupn_keys(data, nrep)[0]
    out = np.full((n, max(nrep, 1)), NIL, dtype=np.uint32)
    for i, h in enumerate(data):
        r = o.lookupn_hash(int(h), nrep)
        out[i, :len(r)] = r
    return out


def device_side(form, n):
    """(keys_ptr, the stride / off_ptr keywords of a *_dev call, tensors to keep alive) or, for
    `hashes`, (None, None, the uint32[n] host array a *_hashes call takes)."""
    import torch
    if form == "hashes":
        return None, None, host_side(form, n)[1]
    if form in _LEAD:
        lead = _LEAD[form]
        buf = torch.zeros(n * 36 + 32, dtype=torch.uint8, device="cuda")
        buf[lead:lead + n * 36] = torch.from_numpy(np.array(_fixed(n)).reshape(-1)).cuda()
        assert buf.data_ptr() % 16 == 0
        return buf.data_ptr() + lead, {}, buf
    if form == "stride20":
        buf = torch.from_numpy(np.array(host_side(form, n)[1]).reshape(-1)).cuda()
        return buf.data_ptr(), {"stride": 20}, buf
    var = _var(n)
    buf = torch.from_numpy(np.frombuffer(b"".join(var) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(k) for k in var])]).astype(np.int64)).cuda()
    return buf.data_ptr(), {"stride": 0, "off_ptr": off.data_ptr()}, (buf, off)
