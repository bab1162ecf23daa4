"""tests/packed_model.py against byte vectors written out by hand from the layout table (include/xrslam_hip.h): they pin the bit
order of the four packings independently of pack / unpack agreeing with each other."""
import numpy as np
import pytest

from tests import packed_model as pk


def rows(*hexbytes):
    return np.array([[int(b, 16) for b in hexbytes]], np.uint8)


def test_mipi10_by_hand():
    # AB CD EF 12 | E4 = 11 10 01 00: pixel 0 takes bits 1:0 = 00, pixel 1 bits 3:2 = 01, pixel 2 = 10, pixel 3 = 11
    b = rows("AB", "CD", "EF", "12", "E4")
    want = [0xAB << 2 | 0, 0xCD << 2 | 1, 0xEF << 2 | 2, 0x12 << 2 | 3]
    assert want == [0x2AC, 0x335, 0x3BE, 0x04B]
    assert pk.unpack(b, 4, pk.MIPI10).tolist() == [want]
    assert pk.pack(np.array([want]), pk.MIPI10).tolist() == b.tolist()
    # a width that ends mid-group still carries the whole group
    assert pk.unpack(b, 3, pk.MIPI10).tolist() == [want[:3]]
    assert pk.pack(np.array([want[:1]]), pk.MIPI10).tolist() == [[0xAB, 0, 0, 0, 0x00]]


def test_mipi12_by_hand():
    # 2 px in 3 bytes: the third byte's low nibble belongs to pixel 0, its high nibble to pixel 1
    b = rows("AB", "CD", "E4", "12", "34", "5F")
    want = [0xAB4, 0xCDE, 0x12F, 0x345]
    assert pk.unpack(b, 4, pk.MIPI12).tolist() == [want]
    assert pk.pack(np.array([want]), pk.MIPI12).tolist() == b.tolist()
    assert pk.unpack(b, 3, pk.MIPI12).tolist() == [want[:3]]


def test_p10_by_hand_crosses_every_byte_phase():
    # samples 0x3FF, 0x000, 0x155, 0x2AA, 0x201 start at bit phases 0, 2, 4, 6, 0: 50 bits, lsb first
    s = [0x3FF, 0x000, 0x155, 0x2AA, 0x201]
    stream = sum(v << (10 * x) for x, v in enumerate(s))
    by_hand = [(stream >> (8 * k)) & 255 for k in range(7)]
    assert by_hand == [0xFF, 0x03, 0x50, 0x95, 0xAA, 0x01, 0x02]
    b = np.array([by_hand], np.uint8)
    assert pk.unpack(b, 5, pk.P10).tolist() == [s]
    assert pk.pack(np.array([s]), pk.P10).tolist() == [by_hand]
    # one sample alone: two bytes, the low byte first
    assert pk.pack(np.array([[0x2C1]]), pk.P10).tolist() == [[0xC1, 0x02]]


def test_p12_by_hand():
    # 0xABC, 0x123, 0xF0E: bytes BC | 3A (low nibble of pixel 1 above the high nibble of pixel 0) | 12 | 0E | 0F
    b = rows("BC", "3A", "12", "0E", "0F")
    want = [0xABC, 0x123, 0xF0E]
    assert pk.unpack(b, 3, pk.P12).tolist() == [want]
    assert pk.pack(np.array([want]), pk.P12).tolist() == b.tolist()


@pytest.mark.parametrize("packing", pk.PACKINGS)
def test_unpack_inverts_pack_for_every_small_width(packing):
    for w in range(1, 10):
        s = pk.random_samples(w, 3, packing, seed=w)
        s[0, :] = (1 << pk.BITS[packing]) - 1
        s[1, :] = 0
        p = pk.pack(s, packing)
        assert p.shape == (3, pk.row_bytes(w, packing))
        np.testing.assert_array_equal(pk.unpack(p, w, packing), s, err_msg="%s, width %d" % (packing, w))
        # bytes after the row's own are not read
        np.testing.assert_array_equal(pk.unpack(pk.padded(p, 5), w, packing), s)


def test_row_bytes():
    assert [pk.row_bytes(w, pk.MIPI10) for w in (1, 4, 5, 8, 752)] == [5, 5, 10, 10, 940]
    assert [pk.row_bytes(w, pk.MIPI12) for w in (1, 2, 3, 752)] == [3, 3, 6, 1128]
    assert [pk.row_bytes(w, pk.P10) for w in (1, 2, 3, 4, 5, 752)] == [2, 3, 4, 5, 7, 940]
    assert [pk.row_bytes(w, pk.P12) for w in (1, 2, 3, 752)] == [2, 3, 5, 1128]


def test_format_numbers_and_their_unpacked_counterparts():
    from tests import bayer_model as bm
    from tests import pixfmt_model as pm
    assert pk.NAMES[32] == "gray10_mipi" and pk.NAMES[35] == "gray12p" and pk.NAMES[40] == "bayer_rggb10_mipi" and pk.NAMES[55] == "bayer_bggr12p"
    assert pk.NAMES[49] == "bayer_grbg10p" and pk.PACKING[49] == pk.P10 and pk.UNPACKED[49] == bm.GRBG16
    assert all(pk.UNPACKED[f] == pm.GRAY16 for f in pk.MONO)
    assert len(pk.FORMATS) == 20


def test_the_gray_value_is_the_samples_top_eight_bits():
    """min(255, v >> (bits - 8)) of a 10 / 12-bit sample: what lets the MIPI forms skip the low-bits byte"""
    for fmt in pk.MONO:
        packing = pk.PACKING[fmt]
        s = pk.random_samples(9, 4, packing, seed=fmt)
        np.testing.assert_array_equal(pk.reduce(pk.pack(s, packing), 9, fmt), s >> (pk.BITS[packing] - 8))
