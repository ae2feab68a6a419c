"""The bed-region loops' dictionaries restated in plain Python, the reference of
tests/test_gpu_region_edges.py (pinned to the oracle's sscs_stage / dcs_stage by tests/test_region_refs.py):
group_refs.group's walk over the completed pairs (consensus_helper.py:455-500) plus what the stages' region
loops delete between regions.

  "sscs" (SSCS_maker.py:312-339): at the end of a region every csn_pair_dict entry with two tags is
      emitted, in dict order, and deleted with its two families' read_dict lists; an entry with one tag
      waits for a later region.
  "per_region" (DCS_maker.py:245-282; singleton_correction.py:278-319 deletes its entries alike): at the end
      of a region every entry is processed and deleted.  The families' read_dict lists go by the DCS
      loop's decisions: every tag's but the one whose duplex partner made the DCS before it.

tag_dict is never deleted from, so a pair that completes a family whose read_dict list is gone reads
read_dict[tag]: KeyError (consensus_helper.py:490).  The walk notes the first such pair and goes on as if
the list were there, as the engine does (it groups first and judges afterwards): everything it reports
is then the engine's view, and `late` holds every family a pair joined after its deletion.  Entries are
numbered in csn_pair_dict insertion order; a name whose entry was deleted starts a new entry (dicts
re-insert at the end, so the numbers stay the dict's order).  Everything is dicts, lists and sets."""
import group_refs as R


def sscs_barcode(qname):
    return qname.split("|")[1]


def duplex_barcode(qname):
    return qname.split("_")[0]


def complement(tag):
    """duplex_tag (consensus_helper.py:639-683): the barcode's halves swapped, the other read number."""
    parts = tag.split("_")
    bc = parts[0]
    if "." in bc:
        k = bc.index(".")
        parts[0] = bc[k + 1:] + "." + bc[:k]
    else:
        parts[0] = bc[len(bc) // 2:] + bc[:len(bc) // 2]
    parts[8] = "R2" if parts[8] == "R1" else "R1"
    return "_".join(parts)


class Regions(R.Grouping):
    """group_refs.Grouping with `names` the entry numbers 0 .. E-1 and `entries` keyed by them."""

    def __init__(self):
        R.Grouping.__init__(self)
        self.entry_name = []      # entry -> its molecule name
        self.entry_region = []    # entry -> the region that started it
        self.entry_done = []      # entry -> the region that gave it its second tag (None: one tag)
        self.entry_of = []        # family -> its entry (None: an orphan tag)
        self.emitted = []         # "sscs": the entries in emission order
        self.error = None         # the first pair that reads a deleted read_dict list
        self.late = []            # (pair, family) of every such read
        self.loop_errors = []     # "per_region": regions whose DCS loop reads a deleted partner

    def emitted_families(self):
        return [f for e in self.emitted for f in self.entries[e]]


def region_loop(pairs, read, mode):
    """pairs: [(rec_first, rec_second, region)] in completion order (pair_refs.pairs), regions rising;
    read(i): the group_refs.Read of record i; mode: "sscs" or "per_region" (duplex names)."""
    assert mode in ("sscs", "per_region")
    barcode = sscs_barcode if mode == "sscs" else duplex_barcode
    g = Regions()
    open_entry = {}      # molecule name -> its entry in csn_pair_dict
    alive = set()        # families with a read_dict list
    used = set()         # duplex_dict

    def end_of_region(region):
        for e in sorted(open_entry.values()):                  # dict order
            fams = g.entries[e]
            if mode == "sscs":
                if len(fams) < 2:
                    continue
                g.emitted.append(e)
                alive.difference_update(fams)
            else:
                for f in fams:
                    tag = g.families[f].tag
                    ds = complement(tag)
                    if ds in used:
                        continue
                    if ds in g.by_tag:
                        if g.by_tag[ds] not in alive:
                            g.loop_errors.append(region)
                        used.add(tag)
                    alive.discard(f)
            del open_entry[g.entry_name[e]]

    current = None
    for p, (a, b, region) in enumerate(pairs):
        if current is not None and region != current:
            assert region > current
            end_of_region(current)
        current = region
        first, second = read(a), read(b)
        bc = barcode(first.qname)
        cigars = R.pair_cigars(first, second)
        name = R.pair_name(first, second, bc, cigars)
        for side, r in enumerate((first, second)):
            e = 2 * p + side
            tag = R.end_tag(r, bc, cigars)
            if tag not in g.by_tag:
                f = g.by_tag[tag] = len(g.families)
                fam = R.Family(tag, name, e, region)
                g.families.append(fam)
                alive.add(f)
                fam.members.append(e)
                fam.held.add(r.content())
                if name not in open_entry:
                    open_entry[name] = len(g.names)
                    g.entries[len(g.names)] = []
                    g.names.append(len(g.names))
                    g.entry_name.append(name)
                    g.entry_region.append(region)
                    g.entry_done.append(None)
                ent = g.entries[open_entry[name]]
                if len(ent) < 2:
                    ent.append(f)
                    g.entry_of.append(open_entry[name])
                    if len(ent) == 2:
                        g.entry_done[open_entry[name]] = region
                else:
                    g.orphans += 1
                    g.entry_of.append(None)
            else:
                f = g.by_tag[tag]
                fam = g.families[f]
                if f not in alive and (p, f) not in g.late[-1:]:
                    g.late.append((p, f))
                    if g.error is None:
                        g.error = p
                if first.content() not in fam.held:
                    fam.members.append(e)
                    fam.held.add(r.content())
                else:
                    g.dropped.add(e)
            fam.slots.append(e)
            g.family_of.append(f)
    if current is not None:
        end_of_region(current)
    return g
