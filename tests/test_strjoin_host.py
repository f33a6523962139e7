"""The foreign table of a STRING-key join on the CPU: yt_strjoin_eval builds it
by the rules of the GPU build — every non-null row claims a slot, the key's
canonical slot holds the match list, null keys chain off the null row — and
probes it with strjoin_probe_slot (strjoin.h), the probe the kernels run.
Checked against a Python dict of lists. No GPU.

Contract under test (include/ytql_gpu.h): from the head row of a probe text
the links enumerate exactly the foreign rows that hold the text's bytes; an
absent text gives -1; null joins null; the empty string is a key and is not
null. Every case runs at hash_bits 64, as a query does, and at hash_bits 3,
where the 8 possible hashes make nearly every probe step meet an equal hash
over different bytes."""
import collections

import numpy as np
import pytest

import ytsaurus_amd as y

HASH_BITS = [64, 3]


def chain(head, nxt, n):
    """rows reachable from head through the links; fails on a cycle"""
    out = []
    r = head
    while r != -1:
        assert 0 <= r < n and len(out) <= n, "broken chain"
        out.append(r)
        r = nxt[r]
    return out


def check(foreign, probes, hash_bits):
    model = collections.defaultdict(list)
    for r, s in enumerate(foreign):
        model[s].append(r)
    head, nxt = y.strjoin_eval(foreign, probes, hash_bits)
    assert len(head) == len(probes) and len(nxt) == len(foreign)
    for i, t in enumerate(probes):
        got = chain(head[i], nxt, len(foreign))
        assert sorted(got) == model.get(t, []), (hash_bits, i, t)
        assert len(set(got)) == len(got)
    return head, nxt


def rand_bytes(rng, n):
    # a small alphabet with NUL in it: collisions of prefix and embedded NULs
    return bytes(rng.choice([0, 0x61, 0x62, 0xFF], n).tolist())


def fuzz_lists(rng, size):
    """foreign list of `size` keys (bytes or None) and the probe texts"""
    base = [rand_bytes(rng, int(rng.integers(0, 41))) for _ in range(size)]
    if size >= 12:
        stem = rand_bytes(rng, 16)
        base[0] = b""                                   # the empty string
        base[1] = b"\x00"                               # embedded NULs
        base[2] = b"\x00\x00"
        base[3] = b"a\x00b"
        base[4] = stem + b"tail-A"                      # share 16 bytes
        base[5] = stem + b"tail-B"
        base[6] = b"same-but-last-x"                    # differ in the last byte
        base[7] = b"same-but-last-y"
        base[8] = b"abc"                                # differ only in length
        base[9] = b"abcd"
        base[10] = base[4]                              # duplicates
        base[11] = b""
    if size >= 40:
        for k in range(12, 40, 3):
            base[k] = base[int(rng.integers(0, 12))]    # more duplicates
    foreign = [None if (size >= 4 and rng.random() < 0.07) else s for s in base]
    near = [s[:-1] + bytes([s[-1] ^ 1]) for s in base if s] + \
           [s + b"\x00" for s in base[:50]] + [s[:-1] for s in base[:50] if s]
    probes = base + near + [rand_bytes(rng, int(rng.integers(0, 41)))
                            for _ in range(60)] + [b"", None, b"\x00"]
    return foreign, probes


@pytest.mark.parametrize("hash_bits", HASH_BITS)
@pytest.mark.parametrize("size", [0, 1, 2, 12, 63, 64, 65, 200, 400])
def test_fuzz_against_a_dict_of_lists(size, hash_bits):
    rng = np.random.default_rng(5000 + size)
    for _ in range(3):
        foreign, probes = fuzz_lists(rng, size)
        check(foreign, probes, hash_bits)


@pytest.mark.parametrize("hash_bits", HASH_BITS)
def test_null_joins_null_and_empty_is_a_key(hash_bits):
    foreign = [b"", None, b"x", None, b"", b"x\x00"]
    head, nxt = check(foreign, [None, b"", b"x", b"x\x00", b"y"], hash_bits)
    assert sorted(chain(head[0], nxt, 6)) == [1, 3]
    assert sorted(chain(head[1], nxt, 6)) == [0, 4]
    assert chain(head[2], nxt, 6) == [2]
    assert chain(head[3], nxt, 6) == [5]
    assert head[4] == -1
    # no null foreign key: a null probe finds nothing; and the other way round
    head, _ = check([b"", b"a"], [None], hash_bits)
    assert head == [-1]
    head, _ = check([None, None], [b"", b"a"], hash_bits)
    assert head == [-1, -1]


@pytest.mark.parametrize("hash_bits", HASH_BITS)
def test_many_rows_of_one_key_land_on_one_list(hash_bits):
    """300 rows of one key hold 300 slots; all of them chain off the first
    slot in probe order, whichever rows claimed the others"""
    foreign = [b"dup"] * 150 + [b"other-%d" % i for i in range(50)] + \
        [b"dup"] * 150
    head, nxt = check(foreign, [b"dup", b"other-7", b"du", b"dupp"], hash_bits)
    assert len(chain(head[0], nxt, len(foreign))) == 300


def test_bad_arguments():
    from ytsaurus_amd import _abi
    out = np.zeros(1, dtype=np.int64)
    ends = np.zeros(1, dtype=np.int64)
    for bits in (0, 65, -1):
        rc = _abi.gpu_lib().yt_strjoin_eval(
            b"", ends.ctypes.data, None, 1, b"", ends.ctypes.data, None, 1,
            bits, out.ctypes.data, out.ctypes.data)
        assert rc == _abi.YT_ERR_INVALID_PLAN
