"""Shared cases of the message-layer tests (test_message77.py, test_gpu_message77.py): the known
vectors, frames built field by field, and the boundary payloads."""
import numpy as np

NTOKENS, MAX22, MAXGRID4 = 2063592, 4194304, 32400

# (payload hex, text)
VECTORS = [
    ("000000204def1a8a1988", "CQ K1ABC FN42"),
    ("09bde3506149dc1faa08", "K1ABC W9XYZ -11"),
    ("0c293b804def1abfaa88", "W9XYZ K1ABC R-09"),
    ("09bde3506149dc1fa4c8", "K1ABC W9XYZ RR73"),
    ("09bde3506149dc1fbd48", "K1ABC W9XYZ -35"),
    ("000046f04def1a8a1988", "CQ DX K1ABC FN42"),
    ("000007e06149dc085648", "CQ 123 W9XYZ EN37"),
    ("0c293b884def1aea1988", "W9XYZ/R K1ABC/R R FN42"),
    ("090c166dbdd62a113590", "G4ABC/P PA9XYZ JO22"),
    ("09bde3501a95851fa508", "K1ABC <...> 73"),
    ("63edcee2a4ae07f50000", "TNX BOB 73 GL"),
    ("2468acf13579bde02540", "123456789ABCDEF012"),
    ("56b001a3a311caa00460", "CQ PJ4/K1ABC"),
    ("f31001a3a311caa00520", "<...> PJ4/K1ABC RR73"),
    ("f31001a3a311caa007a0", "PJ4/K1ABC <...> 73"),
    ("000000011ba611923748", "DE 3DA0XYZ KG53"),
    ("00000015f376e01fa448", "QRZ 3XA7AB"),
]
# call -> (n22, n12, n10)
HASHES = {"K1ABC": (2920267, 2851, 712), "W9XYZ": (3982604, 3889, 972), "PJ4/K1ABC": (1420834, 1387, 346)}


def frame(v77: int) -> bytes:
    """77 bits as a number -> the 10-byte payload (bit 0 = the top bit of byte 0)."""
    assert 0 <= v77 < 1 << 77
    return (v77 << 3).to_bytes(10, "big")


def bits(payload, start: int, length: int) -> int:
    v = int.from_bytes(bytes(payload), "big") >> 3
    return (v >> (77 - start - length)) & ((1 << length) - 1)


N28_K1ABC = bits(bytes.fromhex(VECTORS[0][0]), 29, 28)   # the second call of "CQ K1ABC FN42"


def std_frame(n28a=2, ipa=0, n28b=N28_K1ABC, ipb=0, ir=0, g15=MAXGRID4 + 1, i3=1) -> bytes:
    v = n28a
    for width, x in ((1, ipa), (28, n28b), (1, ipb), (1, ir), (15, g15), (3, i3)):
        v = (v << width) | x
    return frame(v)


def free_frame(f71: int, n3=0) -> bytes:
    return frame((f71 << 6) | (n3 << 3))


def nonstd_frame(h12, n58, iflip=0, nrpt=0, icq=0) -> bytes:
    v = h12
    for width, x in ((58, n58), (1, iflip), (2, nrpt), (1, icq), (3, 4)):
        v = (v << width) | x
    return frame(v)


# (name, payload, expected status, expected text or None, expected (hash, hash_bits) of entry 0 or None)
BOUNDARY = [
    ("n28=3", std_frame(n28a=3), 0, "CQ 000 K1ABC", None),
    ("n28=1002", std_frame(n28a=1002), 0, "CQ 999 K1ABC", None),
    ("n28=1003", std_frame(n28a=1003), 0, "CQ K1ABC", None),
    ("n28=532443", std_frame(n28a=532443), 0, "CQ ZZZZ K1ABC", None),
    ("n28=532444", std_frame(n28a=532444), 2, "", None),
    ("n28=NTOKENS-1", std_frame(n28a=NTOKENS - 1), 2, "", None),
    ("n28=NTOKENS", std_frame(n28a=NTOKENS), 0, "<...> K1ABC", (0, 22)),
    ("n28=NTOKENS+MAX22-1", std_frame(n28a=NTOKENS + MAX22 - 1), 0, "<...> K1ABC", (4194303, 22)),
    # n = 0 is not an empty call: the callsign formula gives c0 = A1[0] = ' ', c1 = A2[0] = '0',
    # c2 = A3[0] = '0' and three blanks, "00" after stripping (c1 and c2 are never blank, so no
    # standard callsign value strips to nothing)
    ("n28=NTOKENS+MAX22", std_frame(n28a=NTOKENS + MAX22), 0, "00 K1ABC", None),
    ("n28=2^28-1", std_frame(n28a=(1 << 28) - 1), 0, "ZZ9ZZZ K1ABC", None),
    ("n28b=532444", std_frame(n28b=532444), 2, "", None),
    ("g15=0", std_frame(g15=0), 0, "CQ K1ABC AA00", None),
    ("g15=32399", std_frame(g15=32399), 0, "CQ K1ABC RR99", None),
    ("g15=32400", std_frame(g15=32400), 2, "", None),
    ("g15=32405", std_frame(g15=32405), 0, "CQ K1ABC -30", None),
    ("g15=32435", std_frame(g15=32435), 0, "CQ K1ABC +00", None),
    ("g15=32485", std_frame(g15=32485), 0, "CQ K1ABC +50", None),
    ("g15=32486", std_frame(g15=32486), 0, "CQ K1ABC -50", None),
    ("g15=32505", std_frame(g15=32505), 0, "CQ K1ABC -31", None),
    ("g15=32506", std_frame(g15=32506), 2, "", None),
    ("g15=32767", std_frame(g15=32767), 2, "", None),
    ("f71=42^13-1", free_frame(42 ** 13 - 1), 0, "?????????????", None),
    ("f71=42^13", free_frame(42 ** 13), 2, "", None),
    ("f71=2^71-1", free_frame((1 << 71) - 1), 2, "", None),
    ("n58=38^11", nonstd_frame(1, 38 ** 11), 2, "", None),
    ("n58=38^11-1", nonstd_frame(5, 38 ** 11 - 1, icq=1), 0, "CQ ///////////", None),
    ("n58=0", nonstd_frame(1, 0), 2, "", None),
    ("i3=6", std_frame(i3=6), 1, "", None),
    ("i3=0,n3=3", free_frame(12345, n3=3), 1, "", None),
    ("telemetry max", free_frame((1 << 71) - 1, n3=5), 0, "7FFFFFFFFFFFFFFFFF", None),
]


def fixed_payloads() -> np.ndarray:
    """[n, 10] uint8: every vector, then every boundary payload."""
    rows = [bytes.fromhex(h) for h, _ in VECTORS] + [p for _, p, _, _, _ in BOUNDARY]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 10).copy()


def random_payloads(n: int, seed: int) -> np.ndarray:
    """[n, 10] uint8 seeded random payloads, byte 9 masked to the 77 bits as a decode carries it."""
    p = np.random.default_rng(seed).integers(0, 256, size=(n, 10), dtype=np.uint8)
    p[:, 9] &= 0xF8
    return p
