"""Named inputs for cc_duplex_join and cc_group (the function-level ABI on caller-given keys) at the edges
their kernels have: chain walks of 1 .. 64 hops around DUPLEX_CHAIN, fan-in, self-partners, the KeyErrors of
both decision kernels, key widths of 1 .. 64 words whose keys differ in one word or one byte, the key table's
size step and the 256-thread launch edge; for cc_group the family-count steps of its sort's `bits` and the
4,096-entry scan tile.

A join case is a partner graph over integer ids (entry i has id i; an id no entry has is an absent partner)
turned into fixed-width byte keys by one of four injective encodings.  Every case carries the path it is
built to take (`parallel`: k_join_decide alone, `serial`: k_join_serial) and whether the reference raises;
tests/test_join_refs.py checks both claims against tests/join_refs.py and the oracle, so the GPU test can
rely on them.  The expected decisions are the oracle's (cc_oracle.dcs_join / sc_join / group_keys) on the
byte keys themselves."""
import numpy as np

import cc_oracle

DUPLEX_CHAIN = 32
HOPS = (1, 2, 31, 32, 33, 64)
WIDTHS = (4, 8, 12, 252, 256)
STYLES = ("mixed", "first", "last", "byte")
JOIN_SIZES = (1, 255, 256, 257, 512, 513, 2048)
GROUP_SIZES = (255, 256, 257, 4095, 4096, 4097)
GROUP_FAMILIES = (1, 2, 255, 256, 257, 1024, 1025)
FAR = 1 << 20          # ids from here on belong to no entry


def encode(ids, width, style="mixed"):
    """(n, width) uint8 keys of non-negative ids, injective per style: `mixed` every word depends on the id,
    `first` / `last` only the first / last word does, `byte` only the final byte (ids < 256)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    kw = width // 4
    assert width == 4 * kw and kw >= 1 and (ids >= 0).all()
    w = np.arange(kw, dtype=np.uint64)[None, :]
    const = (np.uint64(0xA5A5A5A5) ^ (w * np.uint64(0x01010101))) & np.uint64(0xffffffff)
    words = np.repeat(const, len(ids), axis=0)
    v = ids.astype(np.uint64)
    if style == "mixed":
        words = (v[:, None] * np.uint64(0x9E3779B1) + w * np.uint64(0x85EBCA6B)) & np.uint64(0xffffffff)
        words[:, 0] = v
    elif style == "first":
        words[:, 0] = v
    elif style == "last":
        words[:, kw - 1] = v
    else:
        assert style == "byte" and (ids < 256).all()
        words[:, kw - 1] = (words[:, kw - 1] & np.uint64(0x00ffffff)) | (v << np.uint64(24))
    return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(len(ids), width)


def rows_as_bytes(a):
    return [r.tobytes() for r in a]


class JoinCase:
    def __init__(self, name, mode, pid, xid=None, path="parallel", raises=False, width=48, style="mixed", votes=False):
        self.name, self.mode, self.path, self.raises = name, mode, path, raises
        self.width, self.style, self.votes = width, style, votes
        self.pid = [int(x) for x in pid]
        self.xid = None if xid is None else [int(x) for x in xid]
        self.n = len(self.pid)
        self.keys = encode(np.arange(self.n), width, style)
        self.parts = encode(self.pid, width, style)
        self.x = None if xid is None else encode(self.xid, width, style)

    def tags(self):
        return (rows_as_bytes(self.keys), rows_as_bytes(self.parts), [] if self.x is None else rows_as_bytes(self.x))

    def expected(self):
        """The oracle's (decision, partner) rows; raises cc_oracle.OracleError where the reference raises."""
        k, p, x = self.tags()
        return cc_oracle.dcs_join(k, p) if self.mode == 0 else cc_oracle.sc_join(k, p, x)


# ---- chains ----------------------------------------------------------------------------------------------------
def chain(mode, hops, far, base=0):
    """Entries base .. base + hops, each naming the one before it; the first names `far`: nothing
    (`absent`), an entry after the chain (`later`), the chain's own head (`cycle`, DCS) or an SSCS key
    (`sscs`, SC).  `base` entries with absent partners come first."""
    pid = [FAR + i for i in range(base)]
    first = {"absent": FAR + base, "later": base + hops + 1, "cycle": base + hops, "sscs": 2 * FAR}[far]
    pid += [first] + [base + k - 1 for k in range(1, hops + 1)]
    if far == "later":
        pid.append(FAR + base + hops + 1)
    xid = None
    if mode == 1:
        xid = [2 * FAR + 7, 2 * FAR] if far == "sscs" else [2 * FAR + 7]
    name = "%s-chain-%d-%s%s" % ("dcs" if mode == 0 else "sc", hops, far, "-at%d" % base if base else "")
    return JoinCase(name, mode, pid, xid, path="serial" if hops > DUPLEX_CHAIN else "parallel",
                    raises=mode == 0 and far == "absent")


def chain_cases():
    out = []
    for base in (0, 250):
        for h in HOPS:
            out += [chain(0, h, far, base) for far in ("absent", "later", "cycle")]
            out += [chain(1, h, far, base) for far in ("sscs", "absent", "later")]
    return out


# ---- fan-in, self-partners, shared partners ----------------------------------------------------------------------
def dcs_shape_cases():
    out = []
    # entry 20 is named by 0..9 (before it) and 21..30 (after it); it names entry 5, which is in duplex_dict by
    # then, so it is skipped and stays in read_dict.  Entry 35 names a later entry and is named by 36..39 (skipped).
    pid = [20] * 10 + [FAR + i for i in range(10, 20)] + [5] + [20] * 10 + [FAR + i for i in range(31, 35)]
    pid += [41] + [35] * 4 + [FAR + 40, FAR + 41]
    out.append(JoinCase("dcs-fanin", 0, pid))
    # the shared partner has no partner of its own: it leaves read_dict, the entries after it raise
    out.append(JoinCase("dcs-fanin-keyerror", 0, [3, 3, 3, FAR, 3, 3], raises=True))
    # an entry names itself (a DCS with itself); a later entry names it and is skipped
    out.append(JoinCase("dcs-self", 0, [FAR, 1, 1, FAR + 3, 4, 4], path="parallel"))
    # 300 entries all naming entry 299, across the block edge
    out.append(JoinCase("dcs-fanin-300", 0, [299] * 299 + [0]))
    return out


def sc_shape_cases():
    X = 2 * FAR
    out = []
    # two and three entries share a singleton partner that comes after them: all are corrected by it, the partner
    # then pairs with the entry it names and both leave; a sharer after that finds the partner deleted
    out.append(JoinCase("sc-shared-2-later", 1, [2, 2, 0], [X], path="serial"))
    out.append(JoinCase("sc-shared-3-later", 1, [3, 3, 3, 1], [X], path="serial"))
    out.append(JoinCase("sc-shared-3-later-after", 1, [2, 2, 0, 2], [X], path="serial"))
    # the shared partner comes first (corrected by a later entry, so in correction_dict): the first sharer
    # pairs with it and both leave, the second and third sharers find it deleted
    out.append(JoinCase("sc-shared-2-earlier", 1, [4, 0, 0, FAR, FAR + 1], [X], path="serial"))
    out.append(JoinCase("sc-shared-3-earlier", 1, [5, 0, 0, 0, FAR, FAR + 1], [X], path="serial"))
    # the shared partner is uncorrected (deleted at its own turn): no sharer is corrected
    out.append(JoinCase("sc-shared-2-deleted", 1, [FAR, 0, 0], [X], path="serial"))
    # sharers on both sides of a partner that an SSCS corrects: the one before it is corrected by it, the one
    # after it finds it deleted
    out.append(JoinCase("sc-shared-around", 1, [1, X, 1], [X], path="serial"))
    # a shared SSCS key: only the first entry is corrected by it; the others have no singleton partner
    out.append(JoinCase("sc-shared-sscs", 1, [X, X, X, X + 1], [X + 1, X]))
    # ... or the SSCS key is also entry 5's key: the later sharers are corrected by that singleton (fan-in)
    out.append(JoinCase("sc-shared-sscs-single", 1, [5, 5, 5, FAR, FAR + 1, FAR + 2], [5], path="serial"))
    # an SSCS key equal to a singleton key, one entry naming it: the SSCS wins, the singleton is never used
    out.append(JoinCase("sc-sscs-equals-single", 1, [3, FAR, FAR + 1, FAR + 2], [FAR + 9, 3]))
    # an SSCS key equal to the naming entry's own key: corrected by the SSCS, no raise
    out.append(JoinCase("sc-self-with-sscs", 1, [FAR, 1, FAR + 2], [1]))
    # mutual pairs (0, 3) and (1, 2): all four corrected, all four deleted, correction_dict emptied
    out.append(JoinCase("sc-mutual", 1, [3, 2, 1, 0, FAR, FAR + 1], [X]))
    # entries naming a member of a finished mutual pair would share it; a chain beside one: 3 names the
    # uncorrected 2, 4 names 3
    out.append(JoinCase("sc-mutual-then-chain", 1, [1, 0, FAR, 2, 3], [X]))
    # its own complement: the reference's KeyError, raised by the serial kernel; also behind other entries
    out.append(JoinCase("sc-self", 1, [0], [X], path="serial", raises=True))
    out.append(JoinCase("sc-self-late", 1, [FAR, 0, 2, 2], [X], path="serial", raises=True))
    out.append(JoinCase("sc-self-300", 1, [FAR + i for i in range(299)] + [299], [X], path="serial", raises=True))
    # no SSCS side at all (m == 0): x_keys absent and x_keys empty
    out.append(JoinCase("sc-no-sscs", 1, [1, 0, FAR, 2, 5, FAR + 1], None))
    out.append(JoinCase("sc-empty-sscs", 1, [1, 0, FAR, 2, 5, FAR + 1], []))
    return out


# ---- mixed decision sets --------------------------------------------------------------------------------------
def mixed(mode, n, seed, absent=FAR, serial=False, m=None):
    """(pid, xid) of n entries in random order taking every decision, clean in the reference: mutual pairs,
    one-way pairs, two-hop chains, entries without a partner, and (SC) SSCS hits among decoy SSCS keys.
    Absent ids are absent .. absent + n - 1, SSCS ids absent + n .. ; serial adds a 33-hop chain (DCS) or a
    shared partner (SC)."""
    rng = np.random.default_rng(seed)
    order = [int(x) for x in rng.permutation(n)]
    pid = [absent + i for i in range(n)]
    xhits = []
    xbase = absent + n
    if serial:
        if mode == 0:
            c = sorted(order[:DUPLEX_CHAIN + 2])
            order = order[DUPLEX_CHAIN + 2:]
            pid[c[0]] = c[-1]
            for k in range(1, len(c)):
                pid[c[k]] = c[k - 1]
        else:
            a, b, c = order[:3]
            order = order[3:]
            pid[a] = pid[b] = c
    while order:
        r = rng.random()
        if r < 0.35 and len(order) >= 2:
            a, b = order.pop(), order.pop()
            pid[a], pid[b] = b, a                                   # mutual
        elif r < 0.5 and len(order) >= 2:
            a, b = sorted((order.pop(), order.pop()))
            pid[a] = b                                              # one-way onto a later entry
            if mode == 1 and rng.random() < 0.5:
                xhits.append(pid[b])
        elif r < 0.6 and len(order) >= 3 and mode == 0:
            a, b, c = sorted((order.pop(), order.pop(), order.pop()))
            pid[a], pid[b], pid[c] = b, a, b                        # c joins the skipped b
        elif r < 0.6 and len(order) >= 2 and mode == 1:
            a, b = sorted((order.pop(), order.pop()))
            pid[b] = a                                              # b finds a deleted (SSCS-corrected or not)
            if rng.random() < 0.5:
                xhits.append(pid[a])
        elif r < 0.8 and mode == 1:
            xhits.append(pid[order.pop()])                          # SSCS hit
        else:
            order.pop()                                             # no partner
    if mode == 0:
        return pid, None
    m = max(len(xhits), n if m is None else m)
    xid = xhits + [xbase + k for k in range(m - len(xhits))]
    xid = [xid[int(i)] for i in rng.permutation(len(xid))]
    return pid, xid


def size_cases():
    out = []
    for n in JOIN_SIZES:
        for mode in (0, 1):
            for seed in (1, 2, 3):
                pid, xid = mixed(mode, n, 1000 * n + 10 * seed + mode)
                out.append(JoinCase("%s-size-%d-s%d" % ("dcs" if mode == 0 else "sc", n, seed), mode, pid, xid))
    for n in (257, 2048):
        for mode in (0, 1):
            pid, xid = mixed(mode, n, 77 * n + mode, serial=True)
            out.append(JoinCase("%s-size-%d-serial" % ("dcs" if mode == 0 else "sc", n), mode, pid, xid, path="serial"))
    return out


def width_cases():
    """Every width in every encoding: 80 entries (ids < 256 for the final-byte family), both modes."""
    out = []
    for width in WIDTHS:
        for style in STYLES:
            for mode in (0, 1):
                pid, xid = mixed(mode, 80, 5 * width + mode, absent=80, m=40)
                assert max(pid + (xid or [0])) < 256
                out.append(JoinCase("%s-width-%d-%s" % ("dcs" if mode == 0 else "sc", width, style), mode, pid, xid,
                                    width=width, style=style))
    return out


def vote_cases():
    """One serial case per mode for the vote rows: entry i's read is record i of table A, SSCS key k's record
    k of table X."""
    pid, _ = mixed(0, 120, 4242, serial=True)
    sid, xid = mixed(1, 120, 4343, serial=True, m=50)
    return [JoinCase("dcs-vote-serial", 0, pid, None, path="serial", votes=True),
            JoinCase("sc-vote-serial", 1, sid, xid, path="serial", votes=True)]


def join_cases():
    return chain_cases() + dcs_shape_cases() + sc_shape_cases() + size_cases() + width_cases() + vote_cases()


# ---- refusals ------------------------------------------------------------------------------------------------
BAD_KEY_BYTES = (0, 6, 260)


def duplicate_cases():
    """(name, mode, keys, parts, x): a repeated key among the entries, among the SSCS keys, at indices 0 and
    n - 1 of 600 entries."""
    k = encode(np.arange(8), 48)
    p = encode(np.arange(8) + FAR, 48)
    x = encode(np.arange(4) + 2 * FAR, 48)
    dk = k.copy()
    dk[5] = dk[2]
    dx = x.copy()
    dx[3] = dx[0]
    far = encode(np.arange(600), 48, "last")
    far[599] = far[0]
    return [("dup-keys-dcs", 0, dk, p, None), ("dup-keys-sc", 1, dk, p, x), ("dup-x-keys", 1, k, p, dx),
            ("dup-far-apart", 0, far, encode(np.arange(600) + FAR, 48, "last"), None),
            ("dup-far-apart-x", 1, k, p, far)]


# ---- cc_group ------------------------------------------------------------------------------------------------
class GroupCase:
    def __init__(self, name, fam, width=48, style="mixed"):
        self.name, self.width = name, width
        self.fam = [int(f) for f in fam]
        self.keys = encode(self.fam, width, style)
        self.families = len(set(self.fam))

    def expected(self):
        return cc_oracle.group_keys(rows_as_bytes(self.keys))


def group_cases():
    out = [GroupCase("group-one-key", [7]),
           GroupCase("group-width-4", [i % 37 for i in range(500)], width=4),
           GroupCase("group-width-256-last", [(i * 7) % 300 for i in range(700)], width=256, style="last"),
           GroupCase("group-width-256-byte", [(i * 5) % 200 for i in range(700)], width=256, style="byte"),
           GroupCase("group-width-12-first", [(i * 3) % 100 for i in range(300)], width=12, style="first")]
    for n in GROUP_SIZES:
        out.append(GroupCase("group-%d-distinct" % n, np.random.default_rng(n).permutation(n) + 5))
        for F in GROUP_FAMILIES:
            if F > n:
                continue
            # interleaved: family f's members are F apart; labels in a shuffled order so that first-seen
            # order is not key order
            label = np.random.default_rng(31 * n + F).permutation(F) + 1
            out.append(GroupCase("group-%d-F%d-interleaved" % (n, F), [label[i % F] for i in range(n)]))
            # random sizes: every family present, members scattered
            rng = np.random.default_rng(17 * n + F)
            fam = np.concatenate([np.arange(F), rng.integers(0, F, n - F)])
            out.append(GroupCase("group-%d-F%d-random" % (n, F), label[rng.permutation(fam)]))
    return out
