"""The record classes of the binding (hipdec.Levels, Diff, EnergyBlock, Requant, RequantReport, DecimReport): what
as_dict() hands out -- the keys, in order, and the type of every value -- written out here, and from_dict() as its exact
inverse.  Needs no device and no library: the classes are ctypes structures."""
import ctypes

import pytest

# per class: (key, 0 for an int or the length of a list of ints) in the order as_dict() gives them
TABLE = {
    "Levels": [("frames", 0), ("lead_silent", 0), ("trail_silent", 0), ("sum", 8), ("over", 8), ("min", 8), ("max", 8)],
    "Diff": [("frames_a", 0), ("frames_b", 0), ("compared", 0), ("diff_frames", 0), ("first_diff", 0), ("diff_end", 0),
             ("runs", 0), ("diff_values", 8), ("max_abs", 8), ("channels", 0), ("flags", 0)],
    "EnergyBlock": [("sq_lo", 8), ("sq_hi", 8), ("peak", 8), ("frames", 0)],
    "Requant": [("bits_in", 0), ("bits_out", 0), ("mode", 0), ("seed", 0)],
    "RequantReport": [("frames", 0), ("clipped", 8)],
    "DecimReport": [("frames_in", 0), ("frames_out", 0), ("clipped", 8)],
}
HAS_RESERVED = {"EnergyBlock", "Requant"}


def filled(cls):
    """an instance with another value in every byte but those of `reserved`, which are zero"""
    x = cls.from_buffer_copy(bytes((37 * i + 11) & 0xFF for i in range(ctypes.sizeof(cls))))
    if hasattr(x, "reserved"):
        x.reserved = 0
    return x


@pytest.mark.parametrize("name", sorted(TABLE))
def test_as_dict_keys_and_types(pkg, name):
    cls = getattr(pkg.hipdec, name)
    x = filled(cls)
    d = x.as_dict()
    assert sorted(d) == sorted(k for k, _ in TABLE[name])
    for key, length in TABLE[name]:
        v, field = d[key], getattr(x, key)
        if length:
            assert type(v) is list and len(v) == length and all(type(e) is int for e in v), key
            assert v == list(field), key
        else:
            assert type(v) is int and v == field, key
    assert ("reserved" in dict(cls._fields_)) == (name in HAS_RESERVED) and "reserved" not in d
    # nothing of the record is missing from the dict: its fields but `reserved` are the table's, in the table's order
    assert [f for f, _ in cls._fields_ if f != "reserved"] == [k for k, _ in TABLE[name]]
    assert any(v for v in d.values())


@pytest.mark.parametrize("name", sorted(TABLE))
def test_from_dict_is_the_inverse(pkg, name):
    cls = getattr(pkg.hipdec, name)
    x = filled(cls)
    d = x.as_dict()
    back = cls.from_dict(d)
    assert type(back) is cls and bytes(back) == bytes(x) and back.as_dict() == d
    # reserved is zero on the way back, whatever the record it came from carried
    if name in HAS_RESERVED:
        y = filled(cls)
        y.reserved = 0xDEAD
        assert y.as_dict() == d and bytes(cls.from_dict(y.as_dict())) == bytes(x)
    # it reads every key: another value under any one of them is another record
    for key, length in TABLE[name]:
        other = dict(d)
        other[key] = [e ^ 1 for e in d[key]] if length else d[key] ^ 1
        assert bytes(cls.from_dict(other)) != bytes(x), key
    # ... and needs each of them (and, as above, nothing else)
    for key, _ in TABLE[name]:
        with pytest.raises(KeyError):
            cls.from_dict({k: v for k, v in d.items() if k != key})
