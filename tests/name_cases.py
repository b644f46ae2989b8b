"""Deterministic families of member / server names, from 1 byte to 262 bytes, for the tests of the
name-length branches (tests/test_name_cases.py says which branch each family reaches, from the
inputs alone; tests/test_names_*_gpu.py run them on the device). Pure Python, seeded, no device.

Every name is distinct over all families, free of NUL and of bytes JSON would escape. First bytes
are kept apart so that a family's place in address (byte) order is known:
    ragged   '-' '.' '0'..'9' ':' 'a'..'f'      tiny   '1' ':' 'a' 'b'      prefix  'E'
    long_run 'g' (no other family)              edge32 'h' (no other family)
    host     'n'..'z'                           high   'a', 'z' or a byte >= 0xC2
"""
import random

RAGGED_ALPHABET = "0123456789abcdef.:-"
STATUS_WORD = ("alive", "suspect", "faulty", "leave")


def _rng(tag):
    return random.Random("name_cases/" + tag)


def b(name):
    """A name's bytes, the order every table sorts by."""
    return name.encode("utf-8")


def tiny():
    """Every 1-, 2- and 3-byte name over 'a', 'b', ':', '1' (84 names)."""
    abc = "ab:1"
    out = list(abc)
    out += [x + y for x in abc for y in abc]
    out += [x + y + z for x in abc for y in abc for z in abc]
    return out


def ragged():
    """Four names of every length 1..70 over 0-9a-f.:- (280 names), none of them a tiny name."""
    rng = _rng("ragged")
    taken = set(tiny())
    out = []
    for n in range(1, 71):
        got = 0
        while got < 4:
            s = "".join(rng.choice(RAGGED_ALPHABET) for _ in range(n))
            if s in taken:
                continue
            taken.add(s)
            out.append(s)
            got += 1
    return out


def _word(rng, n, alphabet="abcdefghijklmnopqrstuvwxyz0123456789"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def prefix():
    """base[:n] for n = 1..64 (each a prefix of the next); for k = 1..8 and p in 4k-1, 4k, 4k+1
    (0-based: the last byte of one 4-byte sort chunk, the first and the second of the next) a pair
    of 40-byte names that differ at byte p alone; pairs that differ in their last byte alone, at
    lengths around the chunk boundaries."""
    rng = _rng("prefix")
    base = "E" + _word(rng, 63)
    out = [base[:n] for n in range(1, 65)]
    for k in range(1, 9):
        for p in (4 * k - 1, 4 * k, 4 * k + 1):
            stem = "E" + _word(rng, 39)
            out += [stem[:p] + "0" + stem[p + 1:], stem[:p] + "1" + stem[p + 1:]]
    for n in (3, 4, 5, 8, 9, 12, 13, 32, 33, 64):
        stem = "E" + _word(rng, n - 2)
        out += [stem + "x", stem + "y"]
    return out


def pairs_differing_at(names):
    """{byte index: count} over the pairs of equal-length names that differ at one byte alone
    (quadratic; for the tests of this module)."""
    by_len = {}
    for s in names:
        by_len.setdefault(len(b(s)), []).append(b(s))
    out = {}
    for group in by_len.values():
        for i, x in enumerate(group):
            for y in group[i + 1:]:
                d = [j for j in range(len(x)) if x[j] != y[j]]
                if len(d) == 1:
                    out[d[0]] = out.get(d[0], 0) + 1
    return out


def long_run(count=330):
    """`count` names of 90..130 bytes that all start with 'g': one contiguous run in address order."""
    rng = _rng("long_run")
    out = []
    for i in range(count):
        n = 90 + (i * 17) % 41
        out.append("g" + _word(rng, n - 7, "abcdefghijklmnopqrstuvwxyz0123456789.-") + ":%05d" % (20000 + i))
    return out


def edge32(per_len=30):
    """Names of 28..33 bytes that start with 'h': with the byte misalignment sh of a name in the
    address-ordered copy, sh + length lands on both sides of the 32 bytes the checksum writer
    pre-loads (the four ragged names a length are too few to meet every sh)."""
    rng = _rng("edge32")
    return ["h" + _word(rng, n - 1) for n in range(28, 34) for _ in range(per_len)]


def host(per_len=7, lo=200, hi=262):
    """DNS-shaped names, label.label...:port, of every length lo..hi, per_len of each; labels of
    3..23 bytes that start with 'n'..'z'."""
    rng = _rng("host")
    out = []
    for n in range(lo, hi + 1):
        for _ in range(per_len):
            port = ":%d" % rng.randint(1000, 9999)
            room = n - len(port)
            labels = []
            while room > 0:
                want = rng.randint(3, 20)
                if room - want - 1 < 3:  # the last label takes what is left
                    want = room
                labels.append(rng.choice("nopqrstuvwxyz") + _word(rng, want - 1))
                room -= want + 1 if room > want else want
            s = ".".join(labels) + port
            assert len(s) == n, (n, len(s))
            out.append(s)
    return out


def high():
    """Names holding two-byte UTF-8 characters below U+0800 (bytes >= 0x80): unsigned byte order,
    and farmhash's short-string class that reads signed chars."""
    return ["\u00e9", "\u00e9:", "\u00e9:1", "\u00df", "\u07ff", "\u07ffz", "a\u00e9", "a\u07ff1",
            "z\u00fc.host:99", "\u00f1ode.example:3000", "\u00a1\u00a2\u00a3\u00bf", "z\u0100\u017f:8",
            "\u03bb.\u03bc.\u03bd:443"]


FAMILIES = ("tiny", "ragged", "prefix", "long_run", "edge32", "host", "high")


def family(name):
    return globals()[name]()


def c2_style(n):
    """10.a.b.c:208xx, the shape the other device tests use (15..20 bytes)."""
    return ["10.%d.%d.%d:%d" % (i >> 16 & 255, i >> 8 & 255, i & 255, 20800 + i % 100) for i in range(n)]


# ---- the membership sets

INCARNATIONS = [-(1 << 60), -1, 0, 7] + [10 ** k - 1 for k in range(1, 18)] + [10 ** k for k in range(1, 18)] + \
    [1 << 53, (1 << 60) - 1]


def dec_len(x):
    return len(str(int(x)))


def mixed_names():
    """tiny + ragged + prefix + long_run + high + edge32 and 40 host names, shuffled."""
    names = tiny() + ragged() + prefix() + long_run() + high() + edge32() + host()[3::11][:40]
    _rng("mixed").shuffle(names)
    return names


def mixed_batches(names):
    """Three update batches [(indices, statuses, incarnations)] over mixed_names(): all but every
    fifth name with the four statuses in turn and incarnations from INCARNATIONS; then two batches
    over a third and a half of the names with other statuses and incarnations, many of which
    apply and change a piece's digit count."""
    rng = _rng("mixed-batches")
    n = len(names)
    idx = [i for i in range(n) if i % 5 != 4]
    out = [(idx, [j % 4 for j in range(len(idx))], [rng.choice(INCARNATIONS) for _ in idx])]
    for frac in (3, 2):
        sub = sorted(rng.sample(idx, len(idx) // frac))
        out.append((sub, [rng.randrange(4) for _ in sub], [rng.choice(INCARNATIONS) for _ in sub]))
    return out


def checksum_string(state):
    """generateChecksumString restated: state = {name: (status code, incarnation)} of the members
    that exist; sorted by address bytes, address + status + incarnation joined by ';' (bytes)."""
    return b";".join(b(a) + STATUS_WORD[st].encode() + str(int(inc)).encode()
                     for a, (st, inc) in sorted(state.items(), key=lambda kv: b(kv[0])))


def growing_steps():
    """The growing table: four steps [(names to intern, names to update)]; step 2 holds a few 'h'
    names, so that step 3 ('g') raises the longest name and sorts into the middle; step 4 adds
    names that sort before everything held."""
    rng = _rng("growing")
    first = ["!" + _word(rng, n) for n in (1, 2, 3, 9, 30, 75)] + ["!", "!!"]  # '!' sorts before every other name
    steps = [c2_style(400), ragged() + edge32(per_len=5), long_run(), host()[5::9] + first]
    out, held = [], []
    for fam in steps:
        held = held + fam
        out.append((fam, rng.sample(held, (2 * len(held)) // 3)))
    return out


# ---- the ring set

def ring_servers():
    """About 160 servers: half the tiny names, every third ragged name (every length 1..70), 21
    host names and the names with bytes past 0x7F."""
    names = tiny()[::2] + ragged()[::3] + host()[::21] + high()
    # "a" + "10" and "a1" + "0" are one replica string: a token two servers share is owned by
    # whichever the ring's tie rule picks, which is not what these tests are about
    held = set(names)
    return [t for t in names if not any(t[:k] in held and t[k:].isdigit() for k in range(1, len(t)))]


# ---- the wire set

def wire_plan():
    """About 400 issueAs records in 30 messages over ragged + long_run + host names:
    (names, msg_rec_off, rows) with rows[r] = (address, source, status code, incarnation, source
    incarnation, id). Record lengths (comma included) interleave between about 200 and 330 bytes
    (every eighth is longer and carries a host name), and the records 128..191 (one wave of the writer) hold lengths 259, 260 and 261."""
    import uuid
    rng = _rng("wire")
    names = ragged() + long_run() + host()
    by_len = {}
    for s in names:
        by_len.setdefault(len(s), []).append(s)
    fixed = len('{"id":"","source":"","sourceIncarnationNumber":,"address":"","status":"","incarnationNumber":}') + 36
    n_rec, n_msgs = 400, 30
    cuts = sorted(rng.sample(range(1, n_rec), n_msgs - 1))
    rec_off = [0] + cuts + [n_rec]
    last = {c - 1 for c in rec_off[1:]}
    want = {130: 259, 150: 260, 171: 261, 131: 262, 149: 258}
    rows = []
    for r in range(n_rec):
        st = rng.randrange(4)
        inc = rng.choice([1434500000000 + r, 7, 10 ** 15 + r])
        sinc = rng.choice([1434500000000 - r, 99])
        comma = 0 if r in last else 1
        target = want.get(r) or (rng.randint(345, 420) if r % 8 == 5 else rng.randint(200, 330))
        room = target - comma - fixed - len(STATUS_WORD[st]) - dec_len(inc) - dec_len(sinc)
        la = rng.choice([x for x in by_len if 1 <= room - x and (room - x) in by_len])
        a, s = rng.choice(by_len[la]), rng.choice(by_len[room - la])
        rows.append((a, s, st, inc, sinc, str(uuid.UUID(int=rng.getrandbits(128), version=4))))
    return names, rec_off, rows


# ---- the simulator sets

SIM_NOW0_DEFAULT = 1434401518824 + 10 ** 9
SIM_SUSP = 3


def _sim_dead_events(names, rounds):
    """(dead, events): down from round 0 are a tenth of the nodes, neighbours in address order (so
    their pieces, once suspect and faulty, deviate side by side), and the node with the longest name.
    The next neighbour leaves in round 2, the one after it crashes mid-run, and the node with the
    longest name comes back in round 5."""
    n = len(names)
    order = sorted(range(n), key=lambda a: b(names[a]))
    at = n // 3
    cluster = order[at:at + n // 10]
    rest = [a for a in order if a not in cluster]
    longest = max(rest, key=lambda a: (len(b(names[a])), b(names[a])))
    leave, kill = [a for a in order[at + n // 10:] if a != longest][:2]
    dead = [1 if a in cluster or a == longest else 0 for a in range(n)]
    return dead, [[2, "leave", leave], [rounds // 2 - 1, "kill", kill], [5, "revive", longest]]


def sim_case(name):
    """A simulator scenario: dict(names, inc0, dead, now0, rounds, seed, events). About a tenth of
    the nodes are down from round 0; one leaves, one crashes mid-run, one of the down ones comes
    back (it refutes what the others hold of it, at incarnation now0 + 200 * round; the others
    take that over where it is the greater one).
      tiny-65     short pieces; incarnations 1..9, so a refuted piece grows by 12 digits
      ragged-130  every length 1..70
      host-shrink-65 / -130  base pieces of 244..262 bytes, incarnations of 16 digits and
                  now0 = 1000: a refuted piece shrinks by 12 digits to at most 255 bytes
      host-grow-65 / -130    the same names, incarnations 1..9 and the default now0: a refuted
                  piece grows past 255 bytes
      host-band-65  64 names of 222..231 bytes (their suspect and faulty pieces stay at 255 bytes
                  or less) and one of 240 bytes that is never down and joins afresh in round 3,
                  16-digit incarnations and now0 = 1000: its own view then holds its piece at 250
                  bytes over a base piece of 262 and no piece past 255, and no other view holds a
                  deviated piece of it, so no view of the run is sent to the fallback for plen"""
    kind, n = name.rsplit("-", 1)
    n = int(n)
    rng = _rng("sim/" + name)
    now0 = SIM_NOW0_DEFAULT
    if kind == "tiny":
        names = rng.sample(tiny(), n)
        inc0 = [1 + i % 9 for i in range(n)]
    elif kind == "ragged":
        names = ragged()[1::2][:n]
        inc0 = [rng.choice([3, 10 ** 5, 1434401518824 + i, 10 ** 15 + i]) for i in range(n)]
    elif kind == "host-band":
        names = host(per_len=7, lo=222, hi=231)[:n - 1]
        inc0, now0 = [10 ** 15 + i for i in range(n)], 1000
        dead, events = _sim_dead_events(names, 14)
        names = names + [host(per_len=1, lo=240, hi=240)[0]]
        return dict(names=names, inc0=inc0, dead=dead + [0], now0=now0, rounds=14, seed=4000 + n,
                    events=events + [[3, "join", n - 1]])
    else:
        pool = host(per_len=7, lo=222, hi=240)  # + "alive" + 16 digits + ';' = 244..262
        names = pool[::2][:n] if n <= 65 else pool[:n]
        if kind == "host-shrink":
            inc0, now0 = [10 ** 15 + i for i in range(n)], 1000
        else:
            inc0 = [1 + i % 9 for i in range(n)]
    assert len(names) == n and len(set(names)) == n
    rounds = 14
    dead, events = _sim_dead_events(names, rounds)
    return dict(names=names, inc0=inc0, dead=dead, now0=now0, rounds=rounds, seed=4000 + n, events=events)


SIM_CASES = ("tiny-65", "ragged-130", "host-shrink-65", "host-shrink-130", "host-grow-65", "host-grow-130",
             "host-band-65")


def view_string(names, order, st, inc):
    """A view's checksum string (bytes) from its status and incarnation rows; order = the member
    indices in address order."""
    return b";".join(b(names[a]) + STATUS_WORD[int(st[a]) & 3].encode() + str(int(inc[a])).encode() for a in order)


def sim_up_rows(case):
    """up[r][v]: node v is up in round r (events of round r applied)."""
    up = [not d for d in case["dead"]]
    out = []
    for r in range(case["rounds"]):
        for er, kind, v in case["events"]:
            if er == r and kind in ("kill", "revive", "join"):
                up[v] = kind != "kill"
        out.append(list(up))
    return out


_SIM_RUNS = {}


def sim_oracle_run(orc, name):
    """The CPU oracle's run of sim_case(name), once per process: per round the checksums, the
    status, incarnation and ring rows of every node."""
    if name not in _SIM_RUNS:
        import numpy as np
        c = sim_case(name)
        o = orc.Sim(c["names"], c["inc0"], np.array(c["dead"], dtype=np.uint8), seed=c["seed"], susp_rounds=SIM_SUSP,
                    now0=c["now0"], events=c["events"])
        n = len(c["names"])
        run = {"case": c, "ck": [], "st": [], "inc": [], "ring": [], "up": sim_up_rows(c),
               "order": sorted(range(n), key=lambda a: b(c["names"][a]))}
        for _ in range(c["rounds"]):
            o.step()
            run["ck"].append(o.checksums())
            views = [o.view(v) for v in range(n)]
            run["st"].append(np.stack([s for s, _ in views]))
            run["inc"].append(np.stack([i for _, i in views]))
            run["ring"].append(np.stack([o.ring_members(v) for v in range(n)]))
        _SIM_RUNS[name] = run
    return _SIM_RUNS[name]


def sim_piece_stats(run, field_max, chunk=20, group=112):
    """Over every (round, live view, member) whose piece deviates from the base string (another
    status or incarnation): how many have plen > field_max, how many have plen <= field_max < blen
    (blen the base piece's bytes, plen the view's, separator included), the largest blen and name
    length, and the most deviated pieces that start in one `chunk`-byte chunk / `group`-byte group
    of a view's string. Pass 1 decides the fallback per view and the lane kernel per wave, so also:
    band_views, the (round, live view) pairs that hold a band piece and no piece with plen >
    field_max, and band_rounds, the rounds with such a view in which no live view holds a piece
    with plen > field_max (whatever views share a wave)."""
    c = run["case"]
    names, inc0, order = c["names"], c["inc0"], run["order"]
    n = len(names)
    nl = [len(b(s)) for s in names]
    out = dict(over=0, band=0, deviated=0, max_blen=0, max_nl=0, per_chunk=0, per_group=0, band_views=0,
               band_rounds=0)
    for r in range(c["rounds"]):
        round_over = round_band = 0
        for v in range(n):
            if not run["up"][r][v]:
                continue
            st, inc = run["st"][r][v], run["inc"][r][v]
            pos = 0
            chunks, groups = {}, {}
            before = (out["over"], out["band"])
            for k, a in enumerate(order):
                sep = 1 if k + 1 < n else 0
                blen = nl[a] + 5 + dec_len(inc0[a]) + sep
                s = int(st[a]) & 3
                if s == 0 and int(inc[a]) == inc0[a]:
                    pos += blen
                    continue
                plen = nl[a] + len(STATUS_WORD[s]) + dec_len(inc[a]) + sep
                out["deviated"] += 1
                out["over"] += plen > field_max
                out["band"] += plen <= field_max < blen
                out["max_blen"] = max(out["max_blen"], blen)
                out["max_nl"] = max(out["max_nl"], nl[a])
                chunks[pos // chunk] = chunks.get(pos // chunk, 0) + 1
                groups[pos // group] = groups.get(pos // group, 0) + 1
                pos += plen
            out["per_chunk"] = max([out["per_chunk"]] + list(chunks.values()))
            out["per_group"] = max([out["per_group"]] + list(groups.values()))
            view_over, view_band = out["over"] - before[0], out["band"] - before[1]
            out["band_views"] += view_band > 0 and view_over == 0
            round_over += view_over
            round_band += view_band > 0 and view_over == 0
        out["band_rounds"] += round_band > 0 and round_over == 0
    return out
