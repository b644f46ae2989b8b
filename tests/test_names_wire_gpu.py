"""GPU test of the wire encoder on records around and past its 260-byte LDS staging slot: about
400 issueAs records with ids and sources in 30 messages over names of 1..262 bytes
(name_cases.wire_plan; tests/test_name_cases.py shows that lengths 259, 260 and 261 sit in one
wave and that every wave mixes staged and direct records). The bytes against oracle/pywire.py,
and the decoder's columns of those bytes against the input. Exact."""
import numpy as np
import pytest

import name_cases as nc
import pywire

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF


@pytest.mark.parametrize("body", ["array", "ping"])
def test_encode_records_around_the_staging_slot(gpu, body):
    names, rec_off, rows = nc.wire_plan()
    m = gpu.Membership()
    ids = dict(zip(names, m.intern(names)))
    n_msgs = len(rec_off) - 1
    addr = [ids[r[0]] for r in rows]
    src = [ids[r[1]] for r in rows]
    st = [r[2] for r in rows]
    inc = [r[3] for r in rows]
    sinc = [r[4] for r in rows]
    uu = np.stack([np.frombuffer(r[5].encode(), dtype=np.uint8) for r in rows])
    cks = [(2654435761 * (j + 1)) & 0xFFFFFFFF for j in range(n_msgs)]
    msrc = [names[(37 * j) % len(names)] for j in range(n_msgs)]
    msinc = [1434500000000 + j for j in range(n_msgs)]
    blob, off = gpu.wire_encode(m, np.array(rec_off), np.array(addr), np.array(src), np.array(st), np.array(inc),
                                np.array(sinc), uu, form="issueAs", body=body, msg_checksum=cks,
                                msg_source=[ids[a] for a in msrc], msg_source_inc=msinc)
    texts = [blob[int(off[j]):int(off[j + 1])] for j in range(n_msgs)]
    recs = [pywire.issue_as_record(r[5], r[1], r[4], r[0], nc.STATUS_WORD[r[2]], r[3]) for r in rows]
    for j in range(n_msgs):
        want = pywire.body(recs[rec_off[j]:rec_off[j + 1]], body, checksum=cks[j], source=msrc[j], source_inc=msinc[j])
        assert texts[j] == want.encode(), j
    d = gpu.wire_decode(m, texts)
    assert (d["err"] == 0).all()
    assert d["rec_off"].tolist() == rec_off
    assert d["addr"].tolist() == addr and d["src"].tolist() == src
    assert d["status"].tolist() == st and d["inc"].tolist() == inc and d["src_inc"].tolist() == sinc
    for k in (0, 130, 150, 171, len(rows) - 1):
        o = int(d["id_off"][k])
        assert blob[o:o + 36].decode() == rows[k][5]
    if body == "ping":
        assert d["checksum"].tolist() == cks and d["source_inc"].tolist() == msinc
        assert [m.address(int(x)) for x in d["source"]] == msrc
    m.close()
