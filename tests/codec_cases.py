"""One builder of compressed encodings and the answers their decoders owe, shared by the CPU tests (the device source compiled for the
host in both Fq2 layouts, tests/test_codec_cases.py) and the GPU tests (tests/test_gpu_codecs.py): the same bytes and the same expected
status / output on both sides.

Formats (the reference's byte rules, src/utils.rs:84-104 and :130-158):
  G1, 33 B: 0x02 (y even) / 0x03 (y odd) || BE32(x);
  G2, 65 B: 0x0a / 0x0b || BE64(x.im * q + x.re), 0x0b iff u512(y) > u512(-y) with u512(c) = c.im * q + c.re.
Decoder order (oracle/bn254_model.py: g1_from_compressed, g2_from_compressed): G1 range (6), root (6), prefix (3); G2 x.im >= q (6), root
(6), sign byte (3), order-r subgroup (6).  The x.im >= q code is UNPINNED (no reference vector holds one, bn254_amd/csrc/bn254_codec_g2.h);
the cases here follow the model and claim nothing more.

Nothing here imports the library under test or its host build.  The bulk of the valid points are multiples of the generators by hashed
scalars from oracle/c_oracle.py, compressed by the byte rule above: their expected decompression is the bytes they came from.  Every other
expectation is RESTATED here and not taken from the model's decoders, whose f2_sqrt is the device's algorithm: a root exists iff the norm
re^2 + im^2 is a square of Fq (zero counts), the root itself comes from the norm equation (not the complex method) and is accepted only if
its square is the right-hand side, and the sign follows the u512 rule written out below.  tests/test_codec_cases.py asserts that this
restatement and the model's decoders agree on every case.

A case is Case(kind, enc, status, want, pre): want = the uncompressed bytes where status is 0, else None; pre (G2 only) = x || y as the
decoder holds the point BEFORE the subgroup test, for every case whose x splits, has a root and carries a good sign byte — the two
tie-breaks of the sign rule are visible nowhere else, since no such x lies in the subgroup.
"""
import collections
import functools
import hashlib
import random

from oracle import bn254_model as m
from oracle import c_oracle as c

Q, R = m.Q, m.R
ST_OK, ST_ENCODING, ST_MEMBER = m.OK, m.ERR_INVALID_ENCODING, m.ERR_NOT_MEMBER
WAVE = 64
Case = collections.namedtuple("Case", "kind enc status want pre")

G1_KINDS = ("valid random", "edge x", "double fault", "all zero")
G2_KINDS = ("valid random", "division edge", "rhs in Fq, non-residue", "rhs in Fq, residue", "outside the subgroup", "double fault",
            "triple fault", "all zero")
G1_PREFIXES = (0x02, 0x03, 0x00, 0x04, 0x07, 0xFF)
G2_SIGNS = (0x0A, 0x0B, 0x0C)
N_VALID_G1, N_VALID_G2, N_OUTSIDE = 1024, 512, 64


def be(v, n=32):
    return int(v).to_bytes(n, "big")


def _scalar(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "big") % (R - 1) + 1


# ---- the restated arithmetic -------------------------------------------------------------------------------------------------------
def legendre(a):
    a %= Q
    return 0 if a == 0 else (1 if pow(a, (Q - 1) // 2, Q) == 1 else -1)


def fq_root(a):
    """a square root of a residue a (q = 3 mod 4), checked"""
    y = pow(a % Q, (Q + 1) // 4, Q)
    assert y * y % Q == a % Q
    return y


def f2_has_root(a):
    return legendre(a[0] * a[0] + a[1] * a[1]) >= 0


def f2_root(a):
    """some square root of a in Fq2 or None, through the norm: for y = u + v i, u^2 = (re + s) / 2 or (re - s) / 2 with s^2 = norm(a),
    v = im / (2 u); accepted only if its square is a"""
    if not f2_has_root(a):
        return None
    re, im = a[0] % Q, a[1] % Q
    if im == 0:
        y = (fq_root(re), 0) if legendre(re) >= 0 else (0, fq_root(-re))
    else:
        s, half = fq_root(re * re + im * im), (Q + 1) // 2
        t = (re + s) * half % Q
        if legendre(t) < 0:
            t = (re - s) * half % Q
        u = fq_root(t)
        y = (u, im * pow(2 * u, -1, Q) % Q)
    assert m.f2_mul(y, y) == (re, im)
    return y


def u512(v):
    return v[1] * Q + v[0]                                   # utils.rs:40-45


def f2_pick(y, sign):
    """of y and -y the one the sign byte names: 0x0b the greater in the u512 order, anything else the other"""
    yn = ((-y[0]) % Q, (-y[1]) % Q)
    greater, lesser = (y, yn) if u512(y) > u512(yn) else (yn, y)
    return greater if sign == 0x0B else lesser


def twist_rhs(x):
    return m.f2_add(m.f2_mul(m.f2_mul(x, x), x), m.B2)


def g1_compress(u64):
    return bytes([3 if u64[63] & 1 else 2]) + u64[:32]       # utils.rs:84-104


def g2_compress(u128):
    w = [int.from_bytes(u128[i:i + 32], "big") for i in range(0, 128, 32)]
    y, yn = (w[2], w[3]), ((-w[2]) % Q, (-w[3]) % Q)
    return bytes([0x0B if u512(y) > u512(yn) else 0x0A]) + be(w[1] * Q + w[0], 64)       # utils.rs:130-158


def g1_expect(enc):
    """(status, uncompressed bytes or None) of a 33-byte encoding: range, root, prefix"""
    x = int.from_bytes(enc[1:], "big")
    if x >= Q:
        return ST_MEMBER, None
    rhs = (x * x * x + m.B1) % Q
    if legendre(rhs) < 0:
        return ST_MEMBER, None
    if enc[0] not in (2, 3):
        return ST_ENCODING, None
    y = fq_root(rhs)
    if (y & 1) != (enc[0] & 1):
        y = Q - y
    return ST_OK, be(x) + be(y)


@functools.lru_cache(maxsize=None)
def _in_subgroup(p):
    return m.g2_in_subgroup(p)


def g2_split(enc):
    """(x.re, x.im) of the 64 value bytes; x.im may be >= q"""
    im, re = divmod(int.from_bytes(enc[1:], "big"), Q)
    return re, im


def g2_expect(enc, in_subgroup=None):
    """(status, uncompressed bytes or None, pre) of a 65-byte encoding: x.im >= q, root, sign byte, subgroup.  in_subgroup: the
    verdict where the construction of the case knows it (multiples of the generator), else the model's ladder"""
    re, im = g2_split(enc)
    if im >= Q:
        return ST_MEMBER, None, None
    x = (re, im)
    y = f2_root(twist_rhs(x))
    if y is None:
        return ST_MEMBER, None, None
    if enc[0] not in (0x0A, 0x0B):
        return ST_ENCODING, None, None
    y = f2_pick(y, enc[0])
    pre = be(x[0]) + be(x[1]) + be(y[0]) + be(y[1])
    if in_subgroup is None:
        in_subgroup = _in_subgroup((x, y))
    return (ST_OK, pre, pre) if in_subgroup else (ST_MEMBER, None, pre)


def g2_enc(sign, re, im):
    return bytes([sign]) + be(im * Q + re, 64)


# ---- G1 ------------------------------------------------------------------------------------------------------------------------------
G1_EDGE_X = tuple(dict.fromkeys([0, 1, 2, 3, Q - 2, Q - 1, Q, Q + 1, 2 * Q - 1, 1 << 255, (1 << 256) - 1] +
                                [v for k in range(9) for v in ((1 << (29 * k)) - 1, (1 << (29 * k)) + 1)]))     # 29-bit limbs: k = 0 is 0 and 2 again


def _no_root_x(rnd):
    while True:
        x = rnd.randrange(Q)
        if legendre(x * x * x + m.B1) < 0:
            return x


@functools.lru_cache(maxsize=None)
def g1_cases():
    out = []
    gen = c.g1_generator()
    for i in range(N_VALID_G1):
        u = c.g1_mul(gen, be(_scalar(b"codec-g1-%d" % i)))
        out.append(Case("valid random", g1_compress(u), ST_OK, u, None))
    assert {cs.enc[0] for cs in out} == {2, 3}
    for x in G1_EDGE_X:
        for prefix in G1_PREFIXES:
            enc = bytes([prefix]) + be(x)
            st, want = g1_expect(enc)
            out.append(Case("edge x", enc, st, want, None))
    rnd = random.Random(3301)
    for i in range(12):
        prefix = (0x00, 0x04, 0x0A, 0xFF)[i % 4]
        x = rnd.randrange(Q, 1 << 256) if i % 2 else _no_root_x(rnd)                   # range + prefix, root + prefix: the first is reported
        enc = bytes([prefix]) + be(x)
        st, want = g1_expect(enc)
        assert st == ST_MEMBER
        out.append(Case("double fault", enc, st, want, None))
    st, want = g1_expect(bytes(33))
    out.append(Case("all zero", bytes(33), st, want, None))
    return tuple(out)


# ---- G2 ------------------------------------------------------------------------------------------------------------------------------
DIV_COORDS = (0, 1, 2, Q - 2, Q - 1, 1 << 32, (1 << 224) - 1, 1 << 253)
_K_SMALL, _K_LARGE = (1, 2, 3, 1 << 32), (Q - 2, Q - 1, Q + 1, 1 << 254, (1 << 256) - 1, 1 << 256, (1 << 256) + 1, (1 << 256) + Q - 1, 1 << 257)
DIV_WHOLE = tuple(dict.fromkeys([Q * Q - 1, Q * Q, Q * Q + 1, (Q - 1) * Q + (Q - 1), (1 << 512) - 1, 1 << 511, Q * Q + Q - 1] +
                                [k * Q + d for k in _K_SMALL + _K_LARGE for d in (0, 1, -1)]))


def _root_bit(v):
    """of a 512-bit value: None if x.im >= q, else whether the x it splits into has a point on the twist"""
    im, re = divmod(v, Q)
    return None if im >= Q else f2_has_root(twist_rhs((re, im)))


@functools.lru_cache(maxsize=None)
def division_edge_values():
    """the 512-bit values of the division edges.  Among those with x.im < q at least a quarter have a root and a quarter have none
    (a uniform draw gives about half of each); the value after each listed one is added while that does not hold.  Two more conditions,
    each what makes one fault of the division visible in a STATUS: some value whose quotient is exactly q, and some whose quotient
    exceeds 2^256 with its low 256 bits below q, must reduce to an x that has a root — read as x.im = 0 such an encoding would
    decode, with sign byte 0x0c to status 3, where the decoder owes 6."""
    vals = [im * Q + re for re in DIV_COORDS for im in DIV_COORDS] + list(DIV_WHOLE)
    vals = list(dict.fromkeys(vals))

    def census():
        bits = [b for b in map(_root_bit, vals) if b is not None]
        return sum(bits), len(bits) - sum(bits), len(bits)

    step = 1
    while min(census()[:2]) * 4 < census()[2]:
        vals.extend(v + step for v in list(vals) if v + step < 1 << 512 and v + step not in vals)
        step += 1
    for base in (Q * Q, (1 << 256) * Q):                     # quotient == q; quotient == 2^256 (its low 256 bits are 0)
        re = next(r for r in range(64) if f2_has_root(twist_rhs((r, 0))))
        if base + re not in vals:
            vals.append(base + re)
        assert _root_bit(base + re) is None
    return tuple(vals)


CUBE_M = (Q * Q - 1) // 9                                     # v3(q^2 - 1) = 2


@functools.lru_cache(maxsize=None)
def _ninth_root_of_unity():
    k = 2
    while True:
        w = m.f2_pow((k, 1), CUBE_M)
        if m.f2_pow(w, 3) != m.F2_ONE:
            return w
        k += 1


def f2_cube_root(t):
    """a cube root of t in Fq2 or None: one exponentiation by 1/3 mod (q^2 - 1) / 9, then the nine-step search over the 9th roots of unity"""
    if m.f2_pow(t, (Q * Q - 1) // 3) != m.F2_ONE:
        return None
    assert CUBE_M % 3 != 0
    x0, w = m.f2_pow(t, pow(3, -1, CUBE_M)), _ninth_root_of_unity()
    for _ in range(9):
        if m.f2_mul(m.f2_mul(x0, x0), x0) == t:
            return x0
        x0 = m.f2_mul(x0, w)
    raise AssertionError("a cube without a cube root")


@functools.lru_cache(maxsize=None)
def fq_rational_x(want=5):
    """{False: [(c, x)...], True: [...]}: x in Fq2 with x^3 + b' = c in Fq, by whether c is a residue.  c a non-residue: y = +-sqrt(-c) i,
    the alpha == -1 branch of the complex method, sign decided by im; c a residue: y.im == 0, sign decided by re"""
    out = {False: [], True: []}
    cc = 1
    while min(len(v) for v in out.values()) < want:
        cc += 1
        x = f2_cube_root(m.f2_sub((cc, 0), m.B2))
        if x is None:
            continue
        assert twist_rhs(x) == (cc, 0)
        out[legendre(cc) > 0].append((cc, x))
    return out


@functools.lru_cache(maxsize=None)
def twist_x_outside_subgroup():
    rnd, out = random.Random(6502), []
    while len(out) < N_OUTSIDE:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        if f2_has_root(twist_rhs(x)):
            out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g2_cases(not_in_subgroup_hex=None):
    """not_in_subgroup_hex: derived["g2_not_in_subgroup"] (tests/golden/derived_vectors.json), one more point outside the subgroup"""
    out = []

    def add(kind, enc, in_subgroup=None, status=None):
        st, want, pre = g2_expect(enc, in_subgroup)
        assert status is None or st == status, (kind, enc.hex(), st, status)
        out.append(Case(kind, enc, st, want, pre))

    gen = c.g2_generator()
    for i in range(N_VALID_G2):
        u = c.g2_mul(gen, be(_scalar(b"codec-g2-%d" % i)))
        enc = g2_compress(u)
        add("valid random", enc, in_subgroup=True, status=ST_OK)
        assert out[-1].want == u                              # the restated root and sign rule give back the oracle's point
        if i % 8 == 0:                                        # the other root of the same x: the negative, in the subgroup as well
            add("valid random", bytes([0x15 - enc[0]]) + enc[1:], in_subgroup=True, status=ST_OK)
    assert {cs.enc[0] for cs in out} == {0x0A, 0x0B}
    for v in division_edge_values():
        for sign in G2_SIGNS:
            enc = bytes([sign]) + be(v, 64)
            bit = _root_bit(v)
            # 0x0c reads out the has-root bit of the decoded x: 3 with a root, 6 without
            add("division edge", enc, status=None if sign != 0x0C else (ST_ENCODING if bit else ST_MEMBER))
    for residue, kind in ((False, "rhs in Fq, non-residue"), (True, "rhs in Fq, residue")):
        for cc, x in fq_rational_x()[residue]:
            for sign in G2_SIGNS:
                add(kind, g2_enc(sign, *x), status=ST_ENCODING if sign == 0x0C else None)
                if sign != 0x0C:
                    y = (int.from_bytes(out[-1].pre[64:96], "big"), int.from_bytes(out[-1].pre[96:], "big"))
                    assert (y[0] == 0 and y[1] != 0) if not residue else (y[1] == 0 and y[0] != 0)
    xs = list(twist_x_outside_subgroup())
    if not_in_subgroup_hex:
        b = bytes.fromhex(not_in_subgroup_hex)
        xs.append((int.from_bytes(b[:32], "big"), int.from_bytes(b[32:64], "big")))
    for i, x in enumerate(xs):
        add("outside the subgroup", g2_enc(G2_SIGNS[i % 2], *x), status=ST_MEMBER)       # good sign byte: 6 (the cofactor is 2q - r)
        add("outside the subgroup", g2_enc(0x0C if i % 2 else 0x00, *x), status=ST_ENCODING)
    rnd = random.Random(6510)
    no_root = []
    while len(no_root) < 6:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        if not f2_has_root(twist_rhs(x)):
            no_root.append(x)
    valid = [cs for cs in out if cs.kind == "valid random"]
    for i, x in enumerate(no_root):
        add("double fault", g2_enc((0x0C, 0x00, 0xFF)[i % 3], *x), status=ST_MEMBER)                            # root + sign byte
        add("double fault", bytes([(0x0C, 0x02)[i % 2]]) + be((Q + 1 + i) * Q + x[0], 64), status=ST_MEMBER)    # x.im >= q + sign byte
        add("double fault", bytes([0x0C]) + valid[i].enc[1:], in_subgroup=True, status=ST_ENCODING)             # sign byte alone on a valid x, for contrast
        # x.im = q + x.im': neither splits nor (reduced) has a root, bad sign byte
        add("triple fault", bytes([0xFF]) + be((Q + x[1]) * Q + x[0], 64), status=ST_MEMBER)
        add("triple fault", g2_enc(0x0C, *xs[i]), status=ST_ENCODING)                                           # root, BAD sign, outside the subgroup: the sign comes first
    st, want, pre = g2_expect(bytes(65))
    out.append(Case("all zero", bytes(65), st, want, pre))
    return tuple(out)


# ---- layouts of a case list in a batch (waves of 64 lanes) ----------------------------------------------------------------------------
CUTS = (1, 63, 64, 65, 127, 129)


def orders(cases):
    """{name: list of cases}: as built; interleaved so that every wave mixes valid and failing items; and arranged so that whole waves
    hold failing items only and one wave holds a single valid item among 63 failures"""
    cases = list(cases)
    good, bad = [cs for cs in cases if cs.status == ST_OK], [cs for cs in cases if cs.status != ST_OK]
    mixed, gi, bi = [], 0, 0
    for pos in range(len(cases)):                             # the failing items evenly spread
        if bi < len(bad) and (bi * len(cases) <= pos * len(bad) or gi == len(good)):
            mixed.append(bad[bi]); bi += 1
        else:
            mixed.append(good[gi]); gi += 1
    assert len(bad) >= 2 * WAVE - 1 and len(good) >= 2
    solid = bad[:WAVE] + bad[WAVE:2 * WAVE - 1]
    solid.insert(WAVE + 37, good[0])                          # wave 1: one valid item among 63 failures
    solid += bad[2 * WAVE - 1:] + good[1:]
    assert sorted(cs.enc for cs in mixed) == sorted(cs.enc for cs in solid) == sorted(cs.enc for cs in cases)
    return {"as built": cases, "mixed waves": mixed, "failing waves": solid}


def wave_profile(cases):
    """per wave: how many items fail"""
    return [sum(1 for cs in cases[w:w + WAVE] if cs.status != ST_OK) for w in range(0, len(cases), WAVE)]
