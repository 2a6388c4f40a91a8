"""jpr_dataset_model.py against the header's text (include/jpegr.h, the dataset
calls): the search, the containment and the per-stream rules at their edges."""
import jpr_dataset_model as D
import jpr_resize_model as R
import jpr_tensor_model as T

# A 40 x 24 x 3, B 24 x 40 x 2, C 8 x 8 x 1, D 17 x 9 x 4
STREAMS = [(40, 24, 3), (24, 40, 2), (8, 8, 1), (17, 9, 4)]
TABLE = D.table_of(STREAMS)
TOTAL = 10


def test_the_table_is_ascending_and_gap_free():
    assert [t[0] for t in TABLE] == [0, 3, 5, 6]
    assert TABLE[-1][0] + TABLE[-1][3] == TOTAL


def test_every_image_finds_its_stream():
    want = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3)]
    assert [D.locate(TABLE, g) for g in range(TOTAL)] == want


def test_edges():
    """g = 0, each stream's last image and the next one's first, the total, 2^63
    and the largest u64."""
    assert D.locate(TABLE, 0) == (0, 0)
    for s, (image0, _, _, nimg, _) in enumerate(TABLE):
        assert D.locate(TABLE, image0 + nimg - 1) == (s, nimg - 1)
        assert D.locate(TABLE, image0) == (s, 0)
    assert D.locate(TABLE, TOTAL) is None
    assert D.locate(TABLE, 1 << 63) is None
    assert D.locate(TABLE, D.U64) is None


def test_the_search_reads_inside_the_table():
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257):
        table = D.table_of([(8, 8, 1 + k % 3) for k in range(n)])
        total = table[-1][0] + table[-1][3]
        for g in list(range(total + 2)) + [1 << 31, 1 << 32, 1 << 63, D.U64]:
            s, read = D.bisect(table, g)
            assert 0 <= s < n and all(0 <= i < n for i in read)
            assert len(read) <= n.bit_length() + 1
            at = D.locate(table, g)
            assert (at is None) == (g >= total)
            if at is not None:
                assert table[at[0]][0] + at[1] == g and at[1] < table[at[0]][3]


def test_one_stream_of_one_image():
    table = D.table_of([(8, 8, 1)])
    assert D.locate(table, 0) == (0, 0) and D.locate(table, 1) is None
    assert D.locate(D.table_of([(8, 8, 1), (16, 8, 1), (8, 8, 1)]), 1) == (1, 0)


def test_a_gap_in_image0():
    """Images 3 and 4 belong to no stream: bad, and their neighbours found."""
    table = [(0, 40, 24, 3, True), (5, 8, 8, 1, True), (6, 17, 9, 4, True)]
    assert [D.locate(table, g) for g in range(2, 7)] == [(0, 2), None, None, (1, 0), (2, 0)]


def test_a_descending_table_delivers_from_a_containing_stream_or_not_at_all():
    tables = [[(6, 17, 9, 4, True), (5, 8, 8, 1, True), (3, 24, 40, 2, True), (0, 40, 24, 3, True)],
              [(3, 24, 40, 2, True), (0, 40, 24, 3, True), (6, 17, 9, 4, True), (5, 8, 8, 1, True)],
              [(0, 8, 8, 4, True), (0, 8, 8, 4, True), (2, 8, 8, 4, True)]]       # overlapping too
    for table in tables:
        for g in list(range(12)) + [1 << 63]:
            s, read = D.bisect(table, g)
            assert all(0 <= i < len(table) for i in read)
            at = D.locate(table, g)
            if at is not None:
                image0, _, _, nimg, _ = table[at[0]]
                assert image0 <= g < image0 + nimg and at[1] == g - image0


def test_bad_descriptors_take_their_own_rectangles_only():
    for broken in ((24, 40, 0), (0, 40, 2), (24, 0, 2), (24, 40, 2, False), (1 << 31, 1 << 31, 2)):
        table = D.table_of([STREAMS[0], broken, STREAMS[2], STREAMS[3]])
        if broken[2] == 0:                                       # the table stays as the caller built it
            table = [(t[0] + (2 if i > 1 else 0),) + t[1:] for i, t in enumerate(table)]
        rects = [(g, 0, 0, 8, 8, 192 * g) for g in range(TOTAL)]
        got = D.tensor_verdicts(table, rects, 16, 16, 192 * TOTAL)
        assert got == [T.GOOD] * 3 + [T.BAD] * 2 + [T.GOOD] * 5, broken


def test_a_rectangle_is_judged_against_its_own_stream():
    inside_a = (0, 20, 10, 16, 12)                               # fits A's 40 x 24 only
    rects = [(g,) + inside_a[1:] + (1000 * i,) for i, g in enumerate((0, 3, 5, 6))]
    assert D.tensor_verdicts(TABLE, rects, 16, 16, 4000) == [T.GOOD, T.BAD, T.BAD, T.BAD]
    assert D.resize_verdicts(TABLE, rects, 16, 16, 7, 5, 4000) == [R.GOOD, R.BAD, R.BAD, R.BAD]
    # max_w bounds every rectangle, whatever its stream's size
    wide = [(0, 0, 0, 17, 8, 0), (5, 0, 0, 8, 8, 500)]
    assert D.tensor_verdicts(TABLE, wide, 16, 16, 4000) == [T.BAD, T.GOOD]
    # the local image index is what the per-stream rule sees: D's last image is its image 3
    assert D.split(TABLE, [(9, 1, 1, 2, 2, 0), (10, 1, 1, 2, 2, 0)]) == {3: [(0, (3, 1, 1, 2, 2, 0))]}


def test_empty_and_capacity_follow_the_single_stream_rules():
    rects = [(0, 0, 0, 0, 5, 0), (5, 0, 0, 8, 8, 0), (6, 0, 0, 8, 8, 4000 - 192), (7, 0, 0, 8, 8, 4000 - 191),
             (10, 0, 0, 0, 0, 0)]
    assert D.tensor_verdicts(TABLE, rects, 16, 16, 4000) == [T.EMPTY, T.GOOD, T.GOOD, T.BAD, T.BAD]
    assert D.result_words(D.tensor_verdicts(TABLE, rects, 16, 16, 4000)) == [3, 4]
    n = 3 * 7 * 5
    rects = [(0, 0, 0, 0, 5, 0), (5, 0, 0, 8, 8, 0), (6, 0, 0, 8, 8, 4000 - n), (7, 0, 0, 8, 8, 4000 - n + 1)]
    assert D.resize_verdicts(TABLE, rects, 16, 16, 7, 5, 4000) == [R.BAD, R.GOOD, R.GOOD, R.BAD]


def test_a_bad_tile_takes_the_rectangles_of_its_stream_that_touch_it():
    # tile (1, 1) of A's image 0 is tile 6 of A; B's image 0 has a tile 6 too
    rects = [(0, 8, 8, 8, 8, 0), (0, 0, 0, 8, 8, 200), (3, 0, 16, 8, 8, 400), (1, 8, 8, 8, 8, 600)]
    got = D.tensor_verdicts(TABLE, rects, 16, 16, 4000, {0: {6}})
    assert got == [T.BAD, T.GOOD, T.GOOD, T.GOOD]
    assert D.tensor_verdicts(TABLE, rects, 16, 16, 4000, {1: {6}}) == [T.GOOD, T.GOOD, T.BAD, T.GOOD]
