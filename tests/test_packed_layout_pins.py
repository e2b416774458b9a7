"""The bytes of the packed (wave-BSCSR) layout, pinned: a SHA-256 per case over the packet stream, the packet row table, the
partition tables and the info fields that the device-versus-host tests compare (tests/test_gpu_device_pack.py: _same).
tests/golden/packed_layout_pins.json was recorded from the host packer BEFORE the entry codec and the partition-cut rule became
shared by the host and the device packer (csrc/wbscsr.hpp: store_entry, csrc/partition_cuts.hpp): a shared definition changes both
packers together, which the host-versus-device tests cannot see. `python tests/test_packed_layout_pins.py --record` rewrites the
file from the library in the tree -- only ever on purpose, when the format itself changes."""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

from test_gpu_device_pack import EDGE_LAYOUTS, _coo

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_layout_pins.json")
INFO_KEYS = ("nnz", "packed_entries", "packed_bytes", "n_packets", "packet_entries", "n_wave_partitions", "packets_per_partition",
             "precision", "fixed_width")

# name -> (matrix, partition hint)
MATRICES = {
    "uniform 3000x512x40": (lambda pkg: pkg.generate_matrix(3000, 512, 40, "uniform", 2), 4088),
    "gamma 20000x1024x20": (lambda pkg: pkg.generate_matrix(20000, 1024, 20, "gamma", 1), 4088),
    # balanced cuts: the uniform cut leaves 1061 partitions for 1200 waves here, under 31/32 (option value 2) but not under 7/8 ...
    "uniform 40000x512x40, balanced at 2": (lambda pkg: pkg.generate_matrix(40000, 512, 40, "uniform", 6), 1200),
    # ... and under 7/8 here (tests/test_host_mirror.py: test_balanced_cuts_fill_the_waves_asked_for_and_lose_nothing)
    "gamma 30000x1024x20, balanced at 1 and 2": (lambda pkg: pkg.generate_matrix(30000, 1024, 20, "gamma", 2), 1016),
}
for _name, _lens, _cols, _hint in EDGE_LAYOUTS:
    MATRICES[_name] = (lambda pkg, lens=_lens, cols=_cols: _coo(pkg, lens, cols, seed=len(lens)), _hint)

# name -> (precision, fixed_width, nnz_per_lane, TKSPMV_F32_C12)
VALUE_TYPES = {
    "F32 c12": ("F32", 0, 4, "1"), "F32 c16": ("F32", 0, 4, "0"), "F32 x8": ("F32", 0, 8, "1"), "F16": ("F16", 0, 4, "1"),
    "Q1_7": ("Q1_7", 0, 4, "1"), "Q1_7_F32": ("Q1_7_F32", 0, 4, "1"),
    "FIXED 20": ("FIXED", 20, 4, "1"), "FIXED 24": ("FIXED", 24, 4, "1"), "FIXED 32": ("FIXED", 32, 4, "1"),
}
BALANCED = ("0", "1", "2")


def digest(p):
    """SHA-256 over what _same() compares."""
    packets, packet_bytes, pkt_row, part_first, part_count = p.raw()
    h = hashlib.sha256()
    for a, dt in ((packets, np.uint8), (pkt_row, "<u4"), (part_first, "<u4"), (part_count, "<u4")):
        h.update(struct.pack("<Q", len(a)))
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    info = p.info()
    h.update(json.dumps([packet_bytes] + [int(info[k]) for k in INFO_KEYS]).encode())
    return h.hexdigest()


def stored_values(val, precision, width):
    """What decode() returns for fp32 input values: the value type's own rounding (wbscsr.hpp), restated."""
    v = val.astype(np.float64)
    if precision == "F16":
        return val.astype(np.float16).astype(np.float32)
    if precision == "Q1_7":
        return (np.minimum(np.floor(v * 128.0), 255.0) / 128.0).astype(np.float32)
    if precision == "Q1_7_F32":
        return (np.minimum(np.floor(v * 128.0 + 0.5), 255.0) / 128.0).astype(np.float32)
    if precision == "FIXED":  # truncated to `width` bits, left-aligned in a u32, read back as float(u32) * 2^-31
        q = np.floor(v * 2.0 ** (width - 1)).astype(np.uint64) << np.uint64(32 - width)
        return q.astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -31)
    return val


def pack_case(pkg, setenv, m, hint, vt, balanced):
    precision, width, C, c12 = VALUE_TYPES[vt]
    setenv("TKSPMV_F32_C12", c12)
    setenv("TKSPMV_BALANCED_CUTS", balanced)
    return pkg.Packed(m, k=8, nnz_per_lane=C, n_wave_partitions=hint, precision=getattr(pkg, precision), fixed_width=width)


def cases():
    return [(name, vt, b) for name in MATRICES for vt in VALUE_TYPES for b in BALANCED]


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(MATRICES))
def test_host_packer_bytes_are_the_pinned_ones(pkg, pins, monkeypatch, name):
    make, hint = MATRICES[name]
    m = make(pkg)
    for vt, (precision, width, C, _) in VALUE_TYPES.items():
        want = stored_values(m.val, precision, width)
        for b in BALANCED:
            p = pack_case(pkg, monkeypatch.setenv, m, hint, vt, b)
            r, c, v = p.decode()
            assert np.array_equal(r, m.row) and np.array_equal(c, m.col), (name, vt, b)
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), (name, vt, b)
            if "balanced" in name and C == 4:  # the balanced cut really fired: the packets were dealt out, floor or ceil of the mean each
                part_count = p.raw()[4]
                if b == "0":
                    uniform = len(part_count)
                elif b in name.split("balanced at")[1]:
                    assert len(part_count) > uniform and part_count.min() < part_count.max(), (vt, b, len(part_count))
                else:
                    assert len(part_count) == uniform, (vt, b)
            assert digest(p) == pins["|".join((name, vt, b))], (name, vt, b)
            p.close()


def test_the_pins_cover_every_case(pins):
    assert sorted(pins) == sorted("|".join(c) for c in cases()) and len(pins) == 11 * 9 * 3


def test_balanced_cuts_option_is_clamped_to_its_range(pkg, pins, monkeypatch):
    """0..2 is the documented range; -1 cuts like 0 and 3 like 2, as the device packer has always read it (the host packer took
    both for 1 while it parsed the option itself)."""
    for name, flag, like, unlike in (("gamma 30000x1024x20, balanced at 1 and 2", "-1", "0", "1"), ("uniform 40000x512x40, balanced at 2", "3", "2", "1")):
        make, hint = MATRICES[name]
        got = digest(pack_case(pkg, monkeypatch.setenv, make(pkg), hint, "F32 c12", flag))
        assert got == pins["|".join((name, "F32 c12", like))] and got != pins["|".join((name, "F32 c12", unlike))], (name, flag)


def _doctored(path, out, offset, value):
    raw = bytearray(open(path, "rb").read())
    raw[offset:offset + 4] = struct.pack("<I", value)
    with open(out, "wb") as f:
        f.write(raw)
    return str(out)


def test_bad_stream_arguments_are_refused_alike(pkg, tmp_path):
    """One validation (wbscsr.cpp: stream_args_error) behind the host packer, the device packer and load_packed: the packers
    answer ERR_INVALID with its text, a packed file whose header fails it is an "inconsistent header". (The device packer's
    side of this needs a GPU: tests/test_gpu_device_pack.py.)"""
    m = _coo(pkg, [3, 4, 5], 16)
    for kw, text in ((dict(fixed_width=27), "fixed_width must be in [8, 32] for fixed-point values (bit-packed: at most 20 / 26 bits, "
                                            "1024 columns; 26: 4 entries per lane) and 0 otherwise"),
                     (dict(precision=pkg.FIXED, fixed_width=7), "fixed_width must be in [8, 32] for fixed-point values (bit-packed: at most "
                                                                "20 / 26 bits, 1024 columns; 26: 4 entries per lane) and 0 otherwise"),
                     (dict(nnz_per_lane=5), "nnz_per_lane must be 4 or 8")):
        with pytest.raises(pkg.TkspmvError) as e:
            pkg.Packed(m, **kw)
        assert e.value.status == pkg._lib.ERR_INVALID and e.value.message == text, kw
    # the same limits in a file's header: fixed_width at byte 88, entries per lane at byte 16 (wbscsr.cpp: FileHeader)
    good = str(tmp_path / "good.tkspmv")
    pkg.Packed(m, nnz_per_lane=4, precision=pkg.FIXED, fixed_width=24).save(good)  # (the 21..26-bit stream)
    assert pkg.Packed.load(good).info()["fixed_width"] == 24
    for offset, value in ((88, 27), (88, 7), (16, 5), (16, 8)):
        with pytest.raises(pkg.TkspmvError) as e:
            pkg.Packed.load(_doctored(good, tmp_path / "bad.tkspmv", offset, value))
        assert e.value.status == pkg._lib.ERR_IO and "inconsistent header" in e.value.message, (offset, value)


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import _pkg
    pkg, out = _pkg.load(), {}
    for name, (make, hint) in MATRICES.items():
        m = make(pkg)
        for vt in VALUE_TYPES:
            for b in BALANCED:
                out["|".join((name, vt, b))] = digest(pack_case(pkg, os.environ.__setitem__, m, hint, vt, b))
    with open(PINS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "pins written to", PINS)
