"""numpy model of the ring checksum a ringpop node's ring holds (lib/ring/index.js:96-105
computeChecksum): farmhash32 of the sorted server names joined by ';'. It is the value the request
proxy sends along and compares (lib/request-proxy/send.js:135-147, index.js:168-191), and what
rp_sim_ring_checksums reports for every simulated node.

The hash is the CPU oracle's (pyoracle.hash32), which tests/test_oracle.py pins to the reference's
vectors; tests/test_proxy_model.py pins ring_checksum itself to the oracle ring's checksum of the
same server set, a value ring_golden.json pins to the reference."""
import numpy as np

import pyoracle

EMPTY_RING = 0xDC56D17A  # hash32(""): computeChecksum of a ring without servers


def ring_checksum(names, row):
    """The ring checksum of the view whose ring holds names[a] where row[a] != 0."""
    held = sorted(name for name, bit in zip(names, row) if bit)
    return pyoracle.hash32(";".join(held))


def ring_checksums(names, rows, cache=None):
    """uint32 per row of rows[V][len(names)]; equal rows are hashed once (`cache`: a dict the
    caller keeps between calls over the same names)."""
    cache = {} if cache is None else cache
    out = np.zeros(len(rows), dtype=np.uint32)
    for v, row in enumerate(np.asarray(rows) != 0):
        key = row.tobytes()
        if key not in cache:
            cache[key] = ring_checksum(names, row)
        out[v] = cache[key]
    return out
