"""Writes the target files of the reference-CLI fixtures that pin the oracle's `-c eth -e` slots in
groups below 1024 and its `-I` stride path:

  data/eth_endo_batch8.rmd    `-m rmd160 -c eth -e --rmd-batch-size 8` over 1..2^20 (`-t 1`)
  data/eth_endo_batch512.rmd  the same with `--rmd-batch-size 512`
  data/endo_stride.txt        `-m address -l both -e -I 7919` over 2^20 slots from key 1 (`-t 1`)

A group of G < 1024 keys from key K holds one real point, its centre C = (K + G/2) G at slot G/2, and
G - 1 points x = -(C.x + ((i+1)G).x), y = -+((i+1)G).y at the slots G/2 +- (i+1) (see
make_rmd_batch_targets.py).  With -c eth -e the reference probes six slots per point S = (x, y)
(keyhunt.cpp:3524-3536): eth of S, -S, beta S, -beta S, beta S again and -beta^2 S -- five distinct
images, (beta^2 x, +y) is never probed.  The batch files plant, under each of the five images, a
centre, the slots on both sides of a centre and a group's slot 0; all five images of one centre (six
records: beta S hits slots 2 and 4); and one (beta^2 x, +y) row that must not be found.  The two slots
G/2 +- (i+1) share their x, so a row planted for one of them is the negated image of the other: the
reference finds both.  Uses the CPU oracle's primitives (test-only)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import oracle  # noqa: E402

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
BETA2 = BETA * BETA % P
L1 = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
L2 = L1 * L1 % N
START = 1
# the five distinct images as (power of beta, Y negated), in the reference's slot order 0, 1, 2, 3, 5
IMAGES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)]
STRIDE = 7919


def slot_point(G: int, g: int, t: int):
    """(x, y) the reference's walk holds at slot t of group g (groups of G keys from START)."""
    half = G // 2
    cx, cy = oracle.pubkey(START + g * G + half)
    if t == half:
        return cx, cy
    i = t - half - 1 if t > half else half - t - 1
    tx, ty = oracle.pubkey(i + 1)
    return (-(cx + tx)) % P, (P - ty) % P if t > half else ty


def image(pt, e: int, neg: int) -> bytes:
    x, y = pt
    return oracle.eth_address(x * (1, BETA, BETA2)[e] % P, (P - y) % P if neg else y)


def batch_rows(G: int, full: bool):
    half = G // 2
    out = []
    for n, (e, neg) in enumerate(IMAGES if full else IMAGES[1::2]):
        g = 11 + 7 * n
        out.append(image(slot_point(G, g, half), e, neg))           # a centre
        out.append(image(slot_point(G, g + 1, half - 1 - n % (half - 1)), e, neg))   # below a centre
        out.append(image(slot_point(G, g + 2, half + 1 + n % (half - 1)), e, neg))   # above a centre
        out.append(image(slot_point(G, g + 3, 0), e, neg))          # a group's slot 0
        if full:
            out.append(image(slot_point(G, g + 4, G - 1), e, neg))  # and its last slot
    c = slot_point(G, 97, half)
    if full:
        out += [image(c, e, neg) for e, neg in IMAGES]              # one point, all five images
    out.append(image(slot_point(G, 101, half), 2, 0))               # (beta^2 x, +y): never probed
    return out


def stride_rows():
    """Addresses for -l both -e with stride 7919 (slot t is the key 1 + 7919 t): lambda and lambda^2
    multiples of slot keys and negations, compressed and uncompressed; one key between two slots."""
    k = [START + t * STRIDE for t in (0, 511, 512, 1023, 1024, 77777, 500000, (1 << 20) - 1)]
    comp = [L1 * k[0] % N, L2 * k[1] % N, (N - L1 * k[2]) % N, N - k[3], k[7]]
    unc = [L1 * k[4] % N, (N - L2 * k[5]) % N, L2 * k[6] % N, N - k[7], START + 5 * STRIDE + 1]
    out = []
    for key in comp:
        x, y = oracle.pubkey(key)
        out.append(oracle.h160_to_address(oracle.hash160_comp(x, 2 + (y & 1))))
    for key in unc:
        out.append(oracle.h160_to_address(oracle.hash160_uncomp(*oracle.pubkey(key))))
    return out


if __name__ == "__main__":
    for G, fn in ((8, "eth_endo_batch8.rmd"), (512, "eth_endo_batch512.rmd")):
        open(os.path.join(HERE, "data", fn), "w").write("\n".join(r.hex() for r in batch_rows(G, G == 8)) + "\n")
    open(os.path.join(HERE, "data", "endo_stride.txt"), "w").write("\n".join(stride_rows()) + "\n")
