"""jpr_select_model.py against the format restatements: a selection from the
packed stream of a batch is the packed stream of the sub-batch's slot arrays,
in both formats and through both re-codings; forced non-canonical JPT1 modes
survive a copy; bad items and bad tiles become empty records and are counted.
No GPU."""
import numpy as np
import pytest

import jpr_format as J
import jpr_select_model as M
import jpt_format as T
import jpt_inputs as I

DIMS = (40, 24, 4)                       # 4 images of 5 x 3 tiles
PER = 15
NT = 60


def arrays():
    return I.random_slots(NT)


def forced_modes(a):
    """Per stream the loosest legal mode that is not the canonical one, else
    the canonical one."""
    _, meta, table = a
    modes = []
    for t in range(NT):
        row = []
        for c in range(3):
            ents = T.entries(table[t], meta[t, c], c)
            canon = T.canonical_mode(ents)
            other = [md for md in (0, 2, 1) if md != canon and T.mode_legal(ents, md)]
            row.append(other[0] if other else canon)
        modes.append(row)
    return modes


def window_tiles(items, out_w, out_h):
    return [t for it in items for t in M.source_tiles(it, DIMS, out_w, out_h)]


def test_no_source_header_gives_empty_records():
    assert M.select(b"x" * 16, DIMS, [0] * (NT + 1), [(0, 0, 0)], 40, 24)[1] == [16 + 2 * PER + 12 * PER, 1, 0]


@pytest.mark.parametrize("items,out_w,out_h", [
    ([(3, 0, 0), (0, 0, 0), (0, 0, 0), (2, 0, 0)], 40, 24),          # whole images, repeated, shuffled
    ([(1, 8, 8), (2, 16, 0), (0, 0, 16)], 24, 8),                      # windows
    ([(1, 32, 16), (3, 24, 8)], 8, 8), ([(0, 8, 0)], 29, 23)])
def test_selection_is_the_pack_of_the_sub_batch(items, out_w, out_h):
    a = arrays()
    sub = M.sub_arrays(a, window_tiles(items, out_w, out_h))
    odims = (out_w, out_h, len(items))
    plain, tight = J.pack(*a, *DIMS), T.pack(*a, *DIMS)
    for src, fmt, want in ((plain, 0, J.pack(*sub, *odims)), (plain, M.JPR1, J.pack(*sub, *odims)),
                           (plain, M.JPT1, T.pack(*sub, *odims)), (tight, 0, T.pack(*sub, *odims)),
                           (tight, M.JPT1, T.pack(*sub, *odims)), (tight, M.JPR1, J.pack(*sub, *odims))):
        got, res, _ = M.select(src, DIMS, M.offsets_of(src, DIMS), items, out_w, out_h, fmt)
        assert got == want
        assert res == [len(want), J.OK, 0]


def test_forced_modes_survive_a_copy_and_expand_to_plain():
    a = arrays()
    modes = forced_modes(a)
    canon = T.stream_modes(*a).tolist()
    assert sum(m != c for rm, rc in zip(modes, canon) for m, c in zip(rm, rc)) > NT
    forced = T.pack(*a, *DIMS, modes=modes)
    assert forced != T.pack(*a, *DIMS)
    items = [(2, 0, 0), (0, 0, 0)]
    tiles = window_tiles(items, 40, 24)
    sub = M.sub_arrays(a, tiles)
    offs = M.offsets_of(forced, DIMS)
    got, res, _ = M.select(forced, DIMS, offs, items, 40, 24)
    assert got == T.pack(*sub, 40, 24, 2, modes=[modes[t] for t in tiles]) and res[1:] == [J.OK, 0]
    assert M.select(forced, DIMS, offs, items, 40, 24, M.JPT1)[0] == got
    assert M.select(forced, DIMS, offs, items, 40, 24, M.JPR1)[0] == J.pack(*sub, 40, 24, 2)


def test_edge_tables_recode_both_ways():
    a = I.edge_slots()
    a = (a[0], I.clamp(a[1]), a[2])
    dims = (128, 8, 1)
    plain, tight = J.pack(*a, *dims), T.pack(*a, *dims)
    got, res, modes = M.select(plain, dims, M.offsets_of(plain, dims), [(0, 0, 0)], 128, 8, M.JPT1)
    assert got == tight and res == [len(tight), J.OK, 0] and set(modes) == {0, 1, 2}
    got, res, _ = M.select(tight, dims, M.offsets_of(tight, dims), [(0, 0, 0)], 128, 8, M.JPR1)
    assert got == plain and res == [len(plain), J.OK, 0]


def test_bad_items_and_bad_tiles():
    a = arrays()
    plain = J.pack(*a, *DIMS)
    offs = M.offsets_of(plain, DIMS)
    items = [(0, 0, 0), (4, 0, 0), (1, 4, 0), (1, 0, 16), (2, 24, 0), (2, 16, 0), (1, 0, 17),
             (M.U64, 0, 0), (0, M.U64 - 7, 0)]
    got, res, _ = M.select(plain, DIMS, offs, items, 24, 16)
    good = [0, 5]
    assert res[1:] == [2, 0]
    n = len(items) * 6
    assert got[:4] == b"JPR1" and len(got) == res[0] and J.header(got) == (24, 16, len(items))
    sizes = np.frombuffer(got[16:16 + 2 * n], "<u2").reshape(len(items), 6)
    for k in range(len(items)):
        assert (k in good) == bool((sizes[k] != 12).any()), k
    # the good ones alone, from the same stream
    alone = M.select(plain, DIMS, offs, [items[k] for k in good], 24, 16)[0]
    recs = got[16 + 2 * n:]
    pos = [0] + np.cumsum(sizes.reshape(-1)).tolist()
    mine = b"".join(recs[pos[6 * k]:pos[6 * k + 6]] for k in good)
    assert mine == alone[16 + 2 * 12:]
    # untrusted offsets: a decreasing pair, sizes 11 and 1,037, an end past in_len
    bad = list(offs)
    bad[3], bad[4] = bad[4], bad[3]
    got, res, _ = M.select(plain, DIMS, bad, [(0, 0, 0)], 40, 24)
    assert res[1] == J.OK and 1 <= res[2] <= 3                # tile 3; 2 and 4 span two records each
    for delta, count in ((11, 1), (1037, 1)):
        bad = list(offs)
        bad[8] = bad[7] + delta
        res = M.select(plain, DIMS, bad, [(0, 0, 0)], 40, 24)[1]
        assert res[1] == J.OK and res[2] >= count
    bad = list(offs)
    bad[NT] = len(plain) + 1
    assert M.select(plain, DIMS, bad, [(3, 0, 0)], 40, 24)[1][2] == 1
    # re-coding applies the record rules: an offset 11 bytes into a record
    bad = list(offs)
    bad[20] += 11
    res_copy = M.select(plain, DIMS, bad, [(1, 0, 0)], 40, 24)[1]
    res_code = M.select(plain, DIMS, bad, [(1, 0, 0)], 40, 24, M.JPT1)[1]
    assert res_copy[2] <= 2 and res_code[2] == 2              # tiles 19 and 20: no longer records
    # a wrong header: every item bad, the target is the asked one, else JPR1
    for broken in (b"K" + plain[1:], plain[:8] + (32).to_bytes(4, "little") + plain[12:]):
        got, res, _ = M.select(broken, DIMS, offs, [(0, 0, 0), (1, 0, 0)], 8, 8, 0)
        assert got == b"JPR1" + bytes([8, 0, 0, 0, 8, 0, 0, 0, 2, 0, 0, 0, 12, 0, 12, 0]) + bytes(24)
        assert res == [44, 1, 0]
        assert M.select(broken, DIMS, offs, [(0, 0, 0)], 8, 8, M.JPT1)[0][:4] == b"JPT1"


def test_capacity_prefix():
    a = arrays()
    plain = J.pack(*a, *DIMS)
    offs = M.offsets_of(plain, DIMS)
    whole, res, _ = M.select(plain, DIMS, offs, [(1, 0, 0)], 40, 24)
    for cap in (0, 15, 16, 17, len(whole) - 1):
        got, r, _ = M.select(plain, DIMS, offs, [(1, 0, 0)], 40, 24, cap=cap)
        assert got == whole[:cap] and r == res
