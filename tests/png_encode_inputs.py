"""Inputs of the PNG encoder's tests.  Run as a script it writes tests/golden/png_encode/: per
fixture the input pixels (<name>.npz) and the file (<name>.png) whose zlib stream the zlib of the
machine that generated it wrote, through zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE),
framed by rule 1 of tests/png_encode_reference.py.  The files are committed, so no test depends on
the local zlib.

A fixture is designed as scanline bytes and turned into pixels by undoing the Sub filter, so that
runs, symbol counts and block boundaries fall where they are meant to.  generate() counts what the
family reaches (png_encode_reference.Stats) and asserts every item of check_coverage().  Three
items an encoder set up like this cannot reach, with the reason:

  * a fixed block as first or middle block.  Such a block holds 16383 symbols.  The dynamic trees are
    Huffman codes of the block's own counts, so they lose to the fixed code by their header at the most
    (a few hundred bits), while the fixed code pays 4 bits more per match (5-bit distance code against
    1) and, on literals, wastes the 22 % of its code space that belongs to the length codes: thousands
    of bits over 16383 symbols either way.  A search over the families below found none.
  * max_blindex = 3.  Every match has distance 1, so the distance tree always is two codes of length 1,
    length 1 is sent plainly, and bl_order holds it at index 17: max_blindex is 17 or 18.
  * a repeat count of 139 as such: a run of 139 zero lengths is sent as 138 and one plain zero.  What
    is asserted is the run.
"""
import os
import struct
import zlib

import numpy as np

import png_encode_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode")
MAX_FIXTURE_BYTES = 120000


def pixels_of(rows, channels=1):
    """rows: (h, w * channels) filtered bytes (without the filter byte) -> the pixels whose Sub filter
    gives them: (h, w) gray or (h, w, 3) B, G, R"""
    rows = np.asarray(rows, np.uint8)
    h, n = rows.shape
    px = np.cumsum(rows.reshape(h, n // channels, channels).astype(np.uint32), axis=1).astype(np.uint8)
    return px[:, :, 0].copy() if channels == 1 else px[:, :, ::-1].copy()


def one_row(body):
    return pixels_of(np.asarray(body, np.uint8)[None, :])


def runs(lengths, values):
    return np.concatenate([np.full(n, v, np.uint8) for n, v in zip(lengths, values)])


def no_neighbours_equal(n, rng, first_not=1):
    """n noise bytes, none equal to the one in front of it (nor the first to `first_not`)"""
    d = rng.integers(0, 256, n, dtype=np.uint8).astype(np.int32)
    prev = first_not
    for i in range(n):
        if d[i] == prev:
            d[i] = (d[i] + 1 + int(rng.integers(0, 254))) % 256
        prev = d[i]
    return d.astype(np.uint8)


def fibonacci_body():
    """17 byte values at the Fibonacci counts 2, 3, 5, ..., 4181, no two equal neighbours; with the end-of-block
    code and the one filter byte, which count 1 and 1, 19 symbols whose Huffman tree is 18 levels deep"""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    counts = fib[2:]
    order = sorted(range(len(counts)), key=lambda k: -counts[k])
    seq = np.concatenate([np.full(counts[k], 10 + 5 * k, np.uint8) for k in order])
    out = np.zeros(seq.size, np.uint8)
    half = (seq.size + 1) // 2
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    return out


def few_values(n, rng):
    """n bytes of four values, none equal to the one in front of it: literals a dynamic block codes in
    two bits each"""
    d = rng.integers(0, 4, n).astype(np.int32)
    prev = -1
    for i in range(n):
        if d[i] == prev:
            d[i] = (d[i] + 1 + int(rng.integers(0, 2))) % 4
        prev = d[i]
    return (d * 3 + 2).astype(np.uint8)


def value_sets_body(rng):
    """bytes drawn evenly from groups of consecutive values with chosen gaps between the groups: runs
    of equal and of zero code lengths in the literal tree"""
    gaps = [3, 10, 11, 138, 139, 7, 4, 6]
    sizes = [4, 7, 3, 8, 5, 6]
    rng.shuffle(gaps)
    rng.shuffle(sizes)
    used, at = [], 2   # (0 stays unused, 1 is the filter byte)
    for g, n in zip(gaps, sizes):
        at += g
        if at + n > 256:
            break
        used += list(range(at, at + n))
        at += n
    used = np.array(used, np.uint8)
    body = np.repeat(used, int(rng.integers(2, 40)))
    rng.shuffle(body)
    return body


def _designed():
    """name -> pixels"""
    rng = np.random.default_rng(20261020)
    f = {}
    f["gray_1x1"] = np.array([[200]], np.uint8)
    f["rgb_1x1"] = np.array([[[10, 20, 30]]], np.uint8)
    f["gray_w1_h300"] = rng.integers(0, 256, (300, 1), dtype=np.uint8)
    f["rgb_w301_h1"] = rng.integers(0, 4, (1, 301, 3), dtype=np.uint8)
    # runs of every length rule 4 distinguishes; the first continues the filter byte (a run at byte 0),
    # the last reaches the last byte
    lengths = [5, 1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 600, 1, 263, 516, 518, 3]
    f["runs_gray_1row"] = one_row(runs(lengths, [1] + [(7 * k) % 251 + 2 for k in range(1, len(lengths))]))
    # pixels whose Sub difference is 1: one run through every row's filter byte
    f["through_filter_gray_40x30"] = pixels_of(np.ones((30, 40), np.uint8))
    f["through_filter_rgb_21x9"] = pixels_of(np.ones((9, 63), np.uint8), 3)
    f["blank_rgb_37x23"] = np.zeros((23, 37, 3), np.uint8)
    f["noise_rgb_33x17"] = rng.integers(0, 256, (17, 33, 3), dtype=np.uint8)
    f["ramp_rgb_50x20"] = np.stack([np.tile(np.arange(50, dtype=np.uint8) * 5, (20, 1)),
                                    np.tile(np.arange(20, dtype=np.uint8)[:, None] * 3, (1, 50)),
                                    np.full((20, 50), 77, np.uint8)], axis=2)
    # 127 * 129 = 16383 literals: the last block is empty
    body = no_neighbours_equal(126 * 129, rng).reshape(129, 126)
    body[:, 0] = np.where(body[:, 0] == 1, 2, body[:, 0])
    body[1:, 0] = np.where(body[1:, 0] == body[:-1, -1], body[1:, 0] ^ 0x40, body[1:, 0])
    body[:, 1] = np.where(body[:, 1] == body[:, 0], body[:, 1] ^ 0x20, body[:, 1])
    body[:, -1] = np.where(body[:, -1] == 1, 3, body[:, -1])
    body[:, -1] = np.where(body[:, -1] == body[:, -2], body[:, -1] ^ 0x10, body[:, -1])
    f["literals_16383_gray_126x129"] = pixels_of(body)
    f["literals_16384_gray_1row"] = one_row(no_neighbours_equal(16383, rng))
    # stored | dynamic | stored: with the filter byte 16383 noise literals, 16383 literals of four values,
    # 100 of noise
    f["blocks_sds_gray_1row"] = one_row(np.concatenate([no_neighbours_equal(16382, rng), few_values(16383, rng),
                                                        no_neighbours_equal(100, rng, 0)]))
    # a block boundary inside a run: 16381 literals, then a run whose first byte is symbol 16382 and whose first
    # match of 258 closes the block
    f["boundary_in_run_gray_1row"] = one_row(np.concatenate([no_neighbours_equal(16380, rng),
                                                             np.full(1000, 9, np.uint8), [3, 4, 5]]))
    f["fibonacci_gray_1row"] = one_row(fibonacci_body())
    # IDAT payloads: a zlib stream of exactly 8192 bytes, and one of 8193 (a last IDAT of one byte)
    f["idat_8192_gray_1row"] = one_row(no_neighbours_equal(8180, rng))
    f["idat_8193_gray_1row"] = one_row(no_neighbours_equal(8181, rng))
    return f


def _searched(have):
    """seeded candidates, kept when they reach an item no fixture before them reached"""
    out = {}
    want = [("dsd", lambda s: _first_middle_last(s).issuperset({("dynamic", "first"), ("stored", "middle"),
                                                                ("dynamic", "last")}) and _stored_off_byte(s)),
            ("bl_repaired", lambda s: s.repaired_bl),
            ("tie", lambda s: s.tie and "dynamic" in s.block_types or (s.tie and len(s.block_types) == 1)),
            ("one_match", lambda s: s.one_match_block),
            ("rep16_3", lambda s: (16, 3) in s.repeats), ("rep16_6", lambda s: (16, 6) in s.repeats),
            ("rep17_3", lambda s: (17, 3) in s.repeats), ("rep17_10", lambda s: (17, 10) in s.repeats),
            ("rep18_11", lambda s: (18, 11) in s.repeats), ("rep18_138", lambda s: (18, 138) in s.repeats),
            ("run7", lambda s: (False, 7) in s.len_runs or (True, 7) in s.len_runs),
            ("run139", lambda s: (True, 139) in s.len_runs),
            ("blindex18", lambda s: 18 in s.max_blindex)]
    reached = set(k for k, test in want if any(test(s) for s in have))
    missing = []
    for key, test in want:
        if key in reached:
            continue
        found = False
        for seed in range(400):
            rng = np.random.default_rng(1000003 * (want.index((key, test)) + 1) + seed)
            if key == "dsd":
                body = np.concatenate([few_values(16382, rng), no_neighbours_equal(16383, rng, 0),
                                       few_values(300, rng)])
            elif key == "bl_repaired":
                n = 3000 + 500 * (seed % 40)
                body = (rng.integers(0, 256, n, dtype=np.uint8) * (rng.random(n) < 0.02)).astype(np.uint8)
            elif key in ("tie", "one_match"):
                n = int(rng.integers(8, 200))
                body = rng.integers(0, 1 + seed % 7, n, dtype=np.uint8) * 17
            else:
                body = value_sets_body(rng)
            if body.size > 65535:
                continue
            px = one_row(body)
            s = R.Stats()
            R.encode(px, s)
            if test(s):
                name = "search_%s_gray_1row" % key
                out[name] = px
                for k2, t2 in want:
                    if t2(s):
                        reached.add(k2)
                found = True
                break
        if not found:
            missing.append(key)
    return out, missing


def _first_middle_last(s):
    n = len(s.block_types)
    out = set()
    for b, t in enumerate(s.block_types):
        if n >= 3 or b == n - 1:
            out.add((t, "last" if b == n - 1 else "first" if b == 0 else "middle"))
        elif b == 0:
            out.add((t, "first"))
    return out


def _stored_off_byte(s):
    return any(t == "stored" and b > 0 and s.block_bits[b] % 8 != 0 for b, t in enumerate(s.block_types))


def library_file(px):
    """the file whose stream the local zlib writes"""
    px = np.asarray(px)
    h, w = px.shape[:2]
    return R.frame_file(w, h, 1 if px.ndim == 2 else 3, R.zlib_rle_stream(R.scanlines(px)))


def check_coverage(stats, pixels, files):
    """stats: one per fixture; raises on anything of DESIGN 4.15's list the family does not reach"""
    shapes = [p.shape for p in pixels]
    assert (1, 1) in shapes and (1, 1, 3) in shapes
    assert any(len(s) == 2 and s[0] == 1 and s[1] > 1 for s in shapes) and any(s[1] == 1 and s[0] > 1 for s in shapes)
    assert any(((1 + s[1] * (3 if len(s) == 3 else 1)) % 16) for s in shapes)
    # runs
    run_lengths, at_zero, to_end, through = set(), False, False, False
    for p in pixels:
        d = np.frombuffer(R.scanlines(p), np.uint8)
        starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
        lens = np.diff(np.concatenate((starts, [d.size])))
        run_lengths |= set(int(v) for v in lens)
        at_zero |= lens[0] >= 4
        to_end |= lens[-1] >= 4
        row = 1 + p.shape[1] * (3 if p.ndim == 3 else 1)
        through |= p.shape[0] > 1 and any(s < row <= s + n - 1 and n >= 4 for s, n in zip(starts, lens))
    for n in (1, 2, 3, 4, 258, 259, 260, 261, 262):
        assert n in run_lengths, n
    assert max(run_lengths) >= 517 and at_zero and to_end and through
    # blocks
    places = set()
    for s in stats:
        places |= _first_middle_last(s)
    for kind in ("stored", "dynamic"):
        for where in ("first", "middle", "last"):
            assert (kind, where) in places, (kind, where)
    assert ("fixed", "last") in places       # (first and middle: unreachable, see the module's text)
    assert any(_stored_off_byte(s) for s in stats)
    assert any(s.boundary_in_run for s in stats)
    assert any(s.symbols == 16383 and len(s.block_types) == 2 for s in stats)
    assert any(s.symbols == 16384 for s in stats)
    assert any(s.no_match_block for s in stats) and any(s.one_match_block for s in stats)
    assert any(286 in s.lcodes for s in stats) and any(257 in s.lcodes for s in stats)
    assert any(s.repaired_l for s in stats) and any(s.repaired_bl for s in stats)
    repeats, len_runs, blindex = set(), set(), set()
    for s in stats:
        repeats |= s.repeats
        len_runs |= s.len_runs
        blindex |= set(s.max_blindex)
    for want in ((16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)):
        assert want in repeats, want
    assert ((False, 7) in len_runs or (True, 7) in len_runs) and (True, 139) in len_runs
    assert blindex == {17, 18}, blindex      # (3: unreachable, see the module's text)
    assert any(s.tie for s in stats)
    # IDAT layout
    zlens = [struct.unpack(">I", f[33:37])[0] if len(f) < 33 + 12 + 8192 + 12 else None for f in files]
    assert any(z is not None for z in zlens)                                         # one IDAT
    idats = [[struct.unpack(">I", f[k:k + 4])[0] for k in _idat_offsets(f)] for f in files]
    assert any(len(i) == 1 for i in idats) and any(len(i) == 2 for i in idats)
    assert any(i[-1] == 1 and len(i) > 1 for i in idats) and any(i[-1] == 8192 for i in idats)


def _idat_offsets(f):
    out, at = [], 33
    while f[at + 4:at + 8] == b"IDAT":
        out.append(at)
        at += 12 + struct.unpack(">I", f[at:at + 4])[0]
    return out


def generate():
    os.makedirs(GOLDEN, exist_ok=True)
    designed = _designed()
    stats = {}
    for name, px in designed.items():
        stats[name] = R.Stats()
        R.encode(px, stats[name])
    searched, missing = _searched(list(stats.values()))
    assert not missing, "the search did not find: %s" % missing
    for name, px in searched.items():
        stats[name] = R.Stats()
        R.encode(px, stats[name])
    fixtures = dict(designed)
    fixtures.update(searched)
    files = {}
    for name, px in sorted(fixtures.items()):
        data = library_file(px)
        assert data == R.encode(px), name          # the restatement and this machine's zlib agree
        files[name] = data
        assert len(data) <= MAX_FIXTURE_BYTES, (name, len(data))
        with open(os.path.join(GOLDEN, name + ".png"), "wb") as fh:
            fh.write(data)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), pixels=px)
    names = sorted(fixtures)
    check_coverage([stats[n] for n in names], [fixtures[n] for n in names], [files[n] for n in names])
    print("wrote %d fixtures (%d bytes of files) to %s, zlib %s" %
          (len(names), sum(len(v) for v in files.values()), GOLDEN, zlib.ZLIB_RUNTIME_VERSION))


# ---- the committed files ---------------------------------------------------------------------------
def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".png"))


def fixture_bytes(name):
    with open(os.path.join(GOLDEN, name + ".png"), "rb") as f:
        return f.read()


def fixture_pixels(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return z["pixels"]


def zlib_stream_of(data):
    """the joined IDAT payloads of a file this encoder writes"""
    return b"".join(data[at + 8:at + 8 + struct.unpack(">I", data[at:at + 4])[0]] for at in _idat_offsets(data))


def local_zlib_reproduces_the_fixtures():
    """whether this machine's zlib may stand in as the reference for inputs generated at test time"""
    return all(R.zlib_rle_stream(R.scanlines(fixture_pixels(n))) == zlib_stream_of(fixture_bytes(n))
               for n in fixture_names())


def random_frames(count=20, seed=7):
    """seeded frames of three kinds, noise, sparse and ramps; gray and colour; all of one size
    per kind of channel so that they stack"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        colour = k % 2 == 1
        shape = (61, 83, 3) if colour else (61, 83)
        kind = (k // 2) % 3
        if kind == 0:
            px = rng.integers(0, 256, shape, dtype=np.uint8)
        elif kind == 1:
            px = (rng.integers(0, 256, shape, dtype=np.uint8) * (rng.random(shape) < 0.03)).astype(np.uint8)
        else:
            ramp = (np.arange(83)[None, :] * int(rng.integers(1, 4)) + np.arange(61)[:, None] * int(rng.integers(0, 3)))
            px = (ramp[:, :, None] + np.arange(3)[None, None, :] * 40 if colour else ramp).astype(np.uint8)
        out.append(px)
    return out


if __name__ == "__main__":
    generate()
