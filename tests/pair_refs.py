"""pair_dict (consensus_helper.py:426-432) restated in plain Python, the reference of
tests/test_gpu_pair_edges.py (pinned to the oracle's FamilyBuilder.feed by tests/test_pair_refs.py):
walk the stream; the first and second occurrence of a qname form a pair, and so do the third and
fourth; an odd last one stays pending.  Entries that the filters take out (consensus_helper.py:404-420)
take no part.  Everything is integer and string equality."""

# flags whose mate is unmapped, as the reference lists them (consensus_helper.py:410)
MATE_UNMAPPED = frozenset((73, 89, 121, 153, 185, 137))


def passes(qname, flag, delim_filter, badread_file, delim="|"):
    """Whether a stream entry enters pair_dict.  A pass that writes no bad-read file pairs every entry
    (the filters only count); one that does takes out, in this order, a qname without the delimiter
    (when the delimiter is checked at all), an unmapped read, a read whose mate is unmapped, and a
    secondary or supplementary alignment."""
    if not badread_file:
        return True
    if delim_filter and delim not in qname:
        return False
    if flag & 0x4:
        return False
    if flag in MATE_UNMAPPED:
        return False
    if flag & 0x100 or flag & 0x800:
        return False
    return True


def pairs(stream_rec, stream_region, qnames, passes):
    """([(rec_first, rec_second, region_of_second)] in the order of the completing entries, the count
    of qnames left pending).  qnames[i] is stream entry i's qname, passes[i] whether it takes part."""
    pending = {}
    out = []
    for i in range(len(stream_rec)):
        if not passes[i]:
            continue
        q = qnames[i]
        if q in pending:
            out.append((int(pending.pop(q)), int(stream_rec[i]), int(stream_region[i])))
        else:
            pending[q] = stream_rec[i]
    return out, len(pending)
