"""cc_duplex_join's two decision kernels (csrc/cc_engine.hip k_join_decide and k_join_serial) restated in
plain Python over resolved indices, so that tests/test_join_refs.py can say on a machine without a GPU which
of the two decides a case: `parallel` (k_join_decide alone), `serial` (k_join_decide asked for
k_join_serial) or, as the verdict, `error` (the deciding kernel raised the reference's KeyError).

resolve() derives the four index arrays the way k_key_insert / k_key_probe leave them: p[i] / xs[i] the
first key equal to entry i's partner key among the entries / the SSCS keys (-1: none), xfirst[k] the lowest
entry probing SSCS key k, indeg[j] the number of entries probing entry j.  decide() and serial() follow the
kernels statement by statement (one loop turn per thread, the atomicOr'd words as booleans).

This restatement is never the expected value of a GPU test: those are cc_oracle.dcs_join / sc_join /
group_keys.  It only names the path."""
import collections

DUPLEX_CHAIN = 32       # k_join_decide's chain walk gives up after this many hops
KEY_MAX_WORDS = 64      # key_bytes <= 256
TABLE_FLOOR = 1024      # key_table's smallest table; otherwise the first power of two >= 2 n
NONE_FIRST = 0x7fffffff

Result = collections.namedtuple("Result", "path error rows")


def table_size(n):
    size = TABLE_FLOOR
    while size < 2 * n:
        size <<= 1
    return size


def key_args_ok(key_bytes):
    return not (key_bytes <= 0 or (key_bytes & 3) or key_bytes > 4 * KEY_MAX_WORDS)


def resolve(keys, parts, xkeys=()):
    """(p, xs, xfirst, indeg, dup) of byte-string keys; dup: a key (or an SSCS key) repeats (flags[0])."""
    first, dup = {}, False
    for i, k in enumerate(keys):
        if k in first:
            dup = True
        first.setdefault(k, i)
    xfirst_key = {}
    for i, k in enumerate(xkeys):
        if k in xfirst_key:
            dup = True
        xfirst_key.setdefault(k, i)
    n, m = len(keys), len(xkeys)
    p = [first.get(parts[i], -1) for i in range(n)]
    xs = [xfirst_key.get(parts[i], -1) for i in range(n)]
    xfirst = [NONE_FIRST] * max(m, 1)
    indeg = [0] * n
    for i in range(n):
        if xs[i] >= 0:
            xfirst[xs[i]] = min(xfirst[xs[i]], i)
        if p[i] >= 0:
            indeg[p[i]] += 1
    return p, xs, xfirst, indeg, dup


def decide(mode, p, xs, xfirst, indeg, chain=DUPLEX_CHAIN):
    """k_join_decide: (rows, seq, err)."""
    n = len(p)
    rows, seq, err = [], False, False
    for i in range(n):
        d, pr = 0, -1
        if mode == 0:
            x, nc = i, 0
            while True:
                g = p[x]
                present = g >= 0
                if not present or g >= x:
                    break
                if nc == chain:
                    seq = True
                    break
                nc += 1
                x = g
            dx = 0 if present else 1
            for _ in range(nc):
                if dx == 0:
                    dx = 2
                elif dx == 1:
                    err = True
                    dx = 3
                else:
                    dx = 0
            d = dx
            if d == 0:
                pr = p[i]
        else:
            if p[i] >= 0 and indeg[p[i]] > 1:
                seq = True
            x, nc, dx, comp = i, 0, 3, False
            while True:
                s = xs[x] if xs[x] >= 0 and xfirst[xs[x]] == x else -1
                g = p[x]
                if s >= 0:
                    dx = 1
                    break
                if g < 0:
                    dx = 3
                    break
                if g == x:
                    seq = True
                    break
                if g > x:
                    dx, comp = 2, False
                    break
                if nc == chain:
                    seq = True
                    break
                nc += 1
                x = g
            for _ in range(nc):
                deleted = dx == 1 or dx == 3 or (dx == 2 and comp)
                if deleted:
                    dx, comp = 3, False
                else:
                    comp = dx == 2 and not comp
                    dx = 2
            d = 0 if dx == 1 else 1 if dx == 2 else 2
            pr = xs[i] if d == 0 else p[i] if d == 1 else -1
        rows.append((d, pr))
    return rows, seq, err


def serial(mode, p, xs, m):
    """k_join_serial: (rows up to the raise, err)."""
    n = len(p)
    used, gone, xgone = [False] * n, [False] * n, [False] * max(m, 1)
    rows = []
    for i in range(n):
        j, pr = p[i], -1
        if mode == 0:
            if j >= 0 and used[j]:
                d = 2
            else:
                if j >= 0:
                    if gone[j]:
                        return rows, True
                    d, pr = 0, j
                    used[i] = True
                else:
                    d = 1
                gone[i] = True
        else:
            s = xs[i]
            if s >= 0 and not xgone[s]:
                d, pr = 0, s
                xgone[s] = True
                gone[i] = True
            elif j >= 0 and not gone[j]:
                d, pr = 1, j
                used[i] = True
                if used[j]:
                    if j == i:
                        return rows, True
                    gone[i] = gone[j] = True
                    used[i] = used[j] = False
            else:
                d = 2
                gone[i] = True
        rows.append((d, pr))
    return rows, False


def join(mode, keys, parts, xkeys=(), chain=DUPLEX_CHAIN):
    """cc_duplex_join after its argument checks: Result(path, error, rows); rows None where it raises.
    A repeated key is path `invalid`."""
    if mode == 0:
        xkeys = ()
    p, xs, xfirst, indeg, dup = resolve(keys, parts, xkeys)
    rows, seq, err = decide(mode, p, xs, xfirst, indeg, chain)
    if dup:
        return Result("invalid", False, None)
    path = "parallel"
    if seq:
        path = "serial"
        rows, err = serial(mode, p, xs, len(xkeys))
    return Result(path, err, None if err else rows)


def verdict(res):
    return "error" if res.error else res.path
