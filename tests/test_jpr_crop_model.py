"""jpr_crop_model.py against hand-written cases (no GPU): the GPU crop tests
take their verdicts and expected bytes from that model, so it is checked here
on cases worked out by hand."""
import numpy as np

import jpr_crop_model as M

G, B, E = M.GOOD, M.BAD, M.EMPTY
BIG = 1 << 20


def test_items_and_scratch():
    assert [M.items(*a) for a in ((1, 1), (8, 8), (9, 8), (224, 224))] == [4, 4, 6, 841]
    assert M.items(0, 8) == 0 and M.items(8, 0) == 0 and M.items(-3, 8) == 0
    assert M.scratch_bytes(1, 8, 8) == 1040 and M.scratch_bytes(0, 8, 8) == 0
    assert M.scratch_bytes(3, 8, 8) == 3088            # 3 * 1028 = 3084, to whole 16-B chunks


def test_classify_by_hand():
    # a 13 x 11 image, 3 of them, maxima 8 x 6
    def c(*rect, cap=BIG):
        return M.classify(rect, 13, 11, 3, 8, 6, cap)
    assert c(0, 0, 0, 8, 6, 0) == G
    assert c(2, 5, 5, 8, 6, 4) == G                    # x + w = 13, y + h = 11: the far corner
    assert c(3, 0, 0, 1, 1, 0) == B                    # image >= nimg
    assert c(0, 0, 0, 9, 6, 0) == B                    # w > max_w
    assert c(0, 0, 0, 8, 7, 0) == B                    # h > max_h
    assert c(0, 6, 0, 8, 6, 0) == B                    # x + w = 14
    assert c(0, 0, 6, 8, 6, 0) == B                    # y + h = 12
    assert c(0, M.U64, 0, 2, 2, 0) == B                # x + w wraps in 64 bits: exact here
    assert c(0, 0, M.U64 - 1, 2, 2, 0) == B
    assert c(0, 0, 0, 8, 6, 2) == B                    # dst not a multiple of 4
    assert c(0, 0, 0, 8, 6, 0, cap=4 * 48) == G        # exactly fits
    assert c(0, 0, 0, 8, 6, 4, cap=4 * 48) == B
    assert c(0, 0, 0, 8, 6, M.U64 - 3) == B            # dst + 4 w h wraps
    assert c(1 << 60, M.U64, 7, 0, 5, 3) == E          # empty, whatever the rest says
    assert c(0, 0, 0, 5, 0, 1) == E
    assert M.classify((0, 0, 0, 8, 6, 0), 13, 11, 3, 8, 6, BIG, header_ok=False) == B
    assert M.classify((0, 0, 0, 0, 0, 0), 13, 11, 3, 8, 6, BIG, header_ok=False) == B


def test_touched_by_hand():
    # 13 x 11: 2 x 2 tiles an image
    assert M.touched((0, 0, 0, 1, 1, 0), 13, 11) == [0]
    assert M.touched((0, 7, 7, 2, 2, 0), 13, 11) == [0, 1, 2, 3]
    assert M.touched((2, 8, 0, 5, 8, 0), 13, 11) == [9]
    assert M.touched((1, 0, 8, 13, 3, 0), 13, 11) == [6, 7]
    # 520 x 520: 65 x 65 tiles; raster tiles 4095 | 4096 are row 63, columns 0 | 1
    assert M.touched((0, 4, 504, 8, 8, 0), 520, 520) == [4095, 4096]
    assert M.touched((1, 512, 512, 8, 8, 0), 520, 520) == [2 * 4225 - 1]
    assert len(M.touched((0, 7, 7, 64, 48, 0), 520, 520)) == 9 * 7 <= M.items(64, 48)


def test_bad_offset_tiles_by_hand():
    in_len = 1000
    good = [100, 150, 200, 260, 1000 - 700, 1000]      # the last tile: 700 B
    assert M.bad_offset_tiles(good, in_len) == set()
    assert M.bad_offset_tiles([100, 150, 1001, 260, 300, 1000], in_len) == {1, 2}   # past in_len
    assert M.bad_offset_tiles([100, 200, 150, 260, 300, 1000], in_len) == {1}       # decreasing
    assert M.bad_offset_tiles([100, 111, 200, 260, 300, 1000], in_len) == {0}       # 11 B
    assert M.bad_offset_tiles([100, 112, 200, 260, 300, 1000], in_len) == set()     # 12 B
    assert M.bad_offset_tiles([0, 1036, 1048], 2000) == set()
    assert M.bad_offset_tiles([0, 1037, 1049], 2000) == {0}
    assert M.bad_offset_tiles([100, -1, 200], in_len) == {0, 1}                     # all ones as int64


def test_verdicts_results_and_bytes_by_hand():
    # one 4 x 3 image whose pixel (x, y) is (x, y, 10 x + y, 255)
    full = np.zeros((1, 3, 4, 4), np.uint8)
    for y in range(3):
        for x in range(4):
            full[0, y, x] = (x, y, 10 * x + y, 255)
    rects = [(0, 1, 1, 2, 2, 0),          # good: rows (1,1)(2,1) / (1,2)(2,2)
             (0, 0, 0, 0, 9, 99),         # empty
             (0, 3, 0, 2, 1, 16),         # bad: x + w = 5
             (0, 3, 2, 1, 1, 20)]         # good: the last pixel
    own = M.verdicts(rects, 4, 3, 1, 2, 2, 24)
    assert own == [G, E, B, G]
    assert M.result_words(own) == [3, 3]
    assert M.result_words([G, E, G]) == [3, M.U64]
    assert M.result_words([B, B]) == [0, 1]
    before = np.full(24, 0x5A, np.uint8)
    out, unspecified = M.expected(full, rects, own, own, before)
    assert out.tolist() == [1, 1, 11, 255, 2, 1, 21, 255, 1, 2, 12, 255, 2, 2, 22, 255,
                            0x5A, 0x5A, 0x5A, 0x5A, 3, 2, 32, 255]
    assert not unspecified.any() and (before == 0x5A).all()
    # the image's only tile fails: both good rectangles turn bad, their bytes unspecified
    failed = M.verdicts(rects, 4, 3, 1, 2, 2, 24, bad_tiles={0})
    assert failed == [B, E, B, B] and M.result_words(failed) == [1, 1]
    out, unspecified = M.expected(full, rects, failed, own, before)
    assert (out == 0x5A).all()
    assert unspecified.tolist() == [True] * 16 + [False] * 4 + [True] * 4
