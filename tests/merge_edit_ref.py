"""The edit of a merge (include/utree_amd.h: utree_merge_files_edit) restated in plain Python on top of merge_ref: the label edit of one
text, the inputs as the imagined build is fed them (nodes filtered, labels mapped), the expected file -- merge_ref.merge(edited(...)) --
and the expected figures of utree_merge_stats and utree_merge_edit_stats, and the preview's text.

Rules: ranks, and drop / keep / rename as None (no such file) or the file's rule lines -- taxa as bytes, rename lines as (old, new); the
rule on position i stands on line i + 1 of the file."""
from collections import namedtuple

import merge_ref as M

Rules = namedtuple("Rules", "ranks drop keep rename")


class EmptyLabel(ValueError):
    """the edit leaves a label text empty: UTREE_E_FORMAT"""


def rules(ranks=0, drop=None, keep=None, rename=None) -> Rules:
    return Rules(ranks, drop, keep, rename)


def rule_file(lines, eol=b"\n") -> bytes:
    """a drop / keep file (bytes) or a rename file ((old, new)) as the product reads it"""
    return b"".join((l if isinstance(l, bytes) else l[0] + b"\t" + l[1]) + eol for l in lines)


def matches(p: bytes, t: bytes) -> bool:
    """clade match: t is p or begins with p followed by ';'"""
    return t == p or t.startswith(p + b";")


def edit_action(t: bytes, r: Rules):
    """(action, edited text): action is keep | rename | cut | rename+cut | drop; the text of a drop is None"""
    if (r.keep is not None and not any(matches(p, t) for p in r.keep)) or (r.drop is not None and any(matches(p, t) for p in r.drop)):
        return "drop", None
    did = []
    hits = [(old, new) for old, new in (r.rename or ()) if matches(old, t)]
    if hits:
        old, new = max(hits, key=lambda on: len(on[0]))
        t = new + t[len(old):]
        did.append("rename")
    if r.ranks and t.count(b";") >= r.ranks:
        t = M.cut_before(t, r.ranks)
        did.append("cut")
    return "+".join(did) or "keep", t


def edit_label(t: bytes, r: Rules):
    """the edited text, or None when the edit drops the label"""
    return edit_action(t, r)[1]


def edited(inputs, r: Rules, minus=()):
    """the regular inputs as the imagined build is fed them: without the nodes whose label is dropped or whose word a MINUS input holds,
    every other node under its edited label"""
    gone = set(w for db in minus for w, _ in db.nodes)
    out = []
    for db in inputs:
        nodes = []
        for w, lab in db.nodes:
            t = edit_label(lab, r)
            if t is None or w in gone:
                continue
            if not t:
                raise EmptyLabel(lab)
            nodes.append((w, t))
        out.append(M.Db(db.W, db.I, nodes))
    return out


def label_lines_of(db):
    """the distinct label texts of an input written by merge_ref.db_file, in line order"""
    seen = {}
    for _, lab in db.nodes:
        seen.setdefault(lab, None)
    return list(seen)


def unmatched(r: Rules, texts):
    """[(which file: 'drop' | 'keep' | 'rename', line, taxon)] of the rules that match none of `texts`, in the preview's order"""
    out = []
    for which, lines in (("drop", r.drop), ("keep", r.keep), ("rename", r.rename)):
        for i, l in enumerate(lines or ()):
            p = l if isinstance(l, bytes) else l[0]
            if not any(matches(p, t) for t in texts):
                out.append((which, i + 1, p))
    return out


def edit_figures(inputs, r: Rules, minus=(), label_lines=None):
    """utree_merge_edit_stats of utree_merge_files_edit.  label_lines: per input its distinct label texts (default: those its nodes carry)."""
    label_lines = label_lines or [label_lines_of(db) for db in inputs]
    acts = [edit_action(t, r)[0] for ls in label_lines for t in ls]
    gone = set(w for db in minus for w, _ in db.nodes)
    dropped = sum(edit_label(lab, r) is None for db in inputs for _, lab in db.nodes)
    sub = sum(edit_label(lab, r) is not None and w in gone for db in inputs for w, lab in db.nodes)
    return {"n_label_lines": len(acts), "n_labels_dropped": acts.count("drop"), "n_labels_renamed": sum("rename" in a for a in acts),
            "n_labels_cut": sum("cut" in a for a in acts), "n_rules_unmatched": len(unmatched(r, [t for ls in label_lines for t in ls])),
            "n_nodes_dropped": dropped, "n_minus_nodes": sum(len(db.nodes) for db in minus), "n_nodes_subtracted": sub}


def merge(inputs, r: Rules, minus=(), gg=True, I=0, label_lines=None):
    """(the output file's bytes, utree_merge_stats' figures, utree_merge_edit_stats' figures); label_lines as for edit_figures"""
    fed = edited(inputs, r, minus)
    data, stats = M.merge(fed, gg, I)
    es = edit_figures(inputs, r, minus, label_lines)
    stats["n_in_nodes"] = sum(len(db.nodes) for db in inputs)
    assert stats["n_in_nodes"] == sum(len(db.nodes) for db in fed) + es["n_nodes_dropped"] + es["n_nodes_subtracted"]
    return data, stats, es


def preview(files, r: Rules, rule_paths):
    """(the preview's bytes, its figures).  files: per regular input (path, '.ubt' | '.ctr', nodes, [(label text, stated count)] in line
    order, repeated texts included); rule_paths: {'drop' | 'keep' | 'rename': path}."""
    out, texts, acts, dropped = [], [], [], 0
    for path, kind, n, lines in files:
        first = {}
        for t, c in lines:
            first.setdefault(t, c)
        out.append(b"# input\t%s\t%s\t%d\t%d\n" % (path.encode(), kind.encode(), n, len(first)))
        for t, c in first.items():
            a, e = edit_action(t, r)
            if e is not None and not e:
                raise EmptyLabel(t)
            out.append(t + b"\t%d\t" % c + a.encode() + b"\t" + (e or b"") + b"\n")
            texts.append(t)
            acts.append(a)
            dropped += c if a == "drop" else 0
    um = unmatched(r, texts)
    for which, line, p in um:
        out.append(b"# unmatched\t%s\t%d\t" % (rule_paths[which].encode(), line) + p + b"\n")
    return b"".join(out), {"n_label_lines": len(acts), "n_labels_dropped": acts.count("drop"), "n_labels_renamed": sum("rename" in a for a in acts),
                           "n_labels_cut": sum("cut" in a for a in acts), "n_rules_unmatched": len(um), "n_nodes_dropped": dropped,
                           "n_minus_nodes": 0, "n_nodes_subtracted": 0}


# ---------------------------------------------------------------- the edit, case by case ----------------------------------------------------------------
def edit_cases(W: int = 8, I: int = 2):
    """name -> (inputs, rules, minus inputs, gg)"""
    L = M._labels()
    LA, LB, LC, LD = L["LA"], L["LB"], L["LC"], L["LD"]
    GONE, STAY = b"k__A;p__B;c__Gone", b"k__A;p__B;c__Stay;o__S"
    out = {
        # LA and LB are both "k__A;p__B;c__C" after the cut: an equal text changes nothing
        "cut_makes_equal": (M.planted(W, I, [(LA, LB), (LA, None), (None, LB)], 21), rules(ranks=3), (), True),
        # "k__A;p__B;c__C" against "k__A;p__B;c__Q": the cut texts fold to "k__A;p__B", a label no input has
        "cut_makes_fold": (M.planted(W, I, [(LA, LC), (LC, LA), (LA, LA)], 22), rules(ranks=3), (), True),
        # the word is shared with a label that would make it BAD; that side is dropped, so the other side's label stays and nothing is shared
        "one_side_dropped": (M.planted(W, I, [(LA, LD), (LD, LB), (LD, LD), (LA, LB)], 23), rules(drop=[b"k__Z"]), (), True),
        "rename_makes_equal": (M.planted(W, I, [(LA, LB), (LB, LA), (LB, None)], 25), rules(rename=[(LB, LA), (b"k__Own;p__I1", b"k__Own;p__I0")]), (), True),
        "everything_dropped": (M.planted(W, I, [(LA, LB), (LA, LD)], 26), rules(keep=[b"k__Nothing"]), (), True),
        "plain_build_cut": (M.planted(W, I, [(LA, LB), (LA, LC), (LA, None)], 27), rules(ranks=3), (), False),
    }
    # GONE and STAY are both "k__A;p__B" after the cut to two ranks; GONE is dropped (selection sees the original text), so the label
    # "k__A;p__B" is dated by STAY's first carrier, after the labels of the nodes in between
    ins = M.planted(W, I, [(GONE, None), (LD, None), (STAY, None), (GONE, STAY)], 24)
    first = min(w for db in ins for w, _ in db.nodes)
    assert first > 0
    ins[0] = M.Db(W, I, [(first - 1, GONE)] + ins[0].nodes)                  # the very first record carries the dropped text
    out["first_carrier_dropped"] = (ins, rules(ranks=2, drop=[GONE]), (), True)
    # a MINUS word that every input holds, MINUS words that one input holds, and MINUS words of its own; the first node of input 0 is
    # subtracted, so its label is dated by its next carrier
    ins = M.planted(W, I, [(LA, LB), (LA, LA), (LC, None), (None, LD)], 28)
    a, b = ins
    mw = sorted(set([a.nodes[0][0], a.nodes[7][0], b.nodes[-1][0]] + [w for w, _ in a.nodes if (w, LA) in b.nodes or (w, LB) in b.nodes][:1]
                    + [w ^ 1 for w, _ in a.nodes[10:20]]))
    out["minus"] = (ins, rules(), (M.Db(W, 4 if I == 2 else 2, [(w, b"k__Host") for w in mw]),), True)
    return out
