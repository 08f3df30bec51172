"""The numpy Philox4x32-10 the GPU tests compare the library's generators with (tests/philox_ref.py) against the
known-answer vectors of the Random123 distribution (kat_vectors, `philox4x32 10`).  No GPU."""
import numpy as np

import philox_ref

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = philox_ref.philox4x32_10([ctr], key)[0]
        assert [int(v) for v in got] == list(want), ([hex(int(v)) for v in got], [hex(v) for v in want])
    # the same three as one batch with per-row keys
    got = philox_ref.philox4x32_10([k[0] for k in KAT], [k[1] for k in KAT])
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))


def test_stream_layout():
    """stream(): the index fills counter words 0-1, the second value words 2-3, the seed the key."""
    seed, second, first = 0x0123456789ABCDEF, (5 << 32) | 7, (1 << 32) - 1
    got = philox_ref.stream(seed, second, first, 2)
    want = philox_ref.philox4x32_10([(0xFFFFFFFF, 0, 7, 5), (0, 1, 7, 5)], (0x89ABCDEF, 0x01234567))
    assert np.array_equal(got, want)
