"""Philox4x32-10 in Python integers, from the published definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC'11, section 3.3 and the Random123 reference tables).  A helper for the dropout known-answer tests, not a
conftest; it shares nothing with the kernel.

One round on the counter (c0, c1, c2, c3) with the round key (k0, k1):
    (hi0, lo0) = M0 * c0,  (hi1, lo1) = M1 * c2          (32 x 32 -> 64 bit products, split into halves)
    counter'   = (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
and the key is bumped by the Weyl constants (W0, W1) between rounds; ten rounds in all."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two.  Returns the four output words as a tuple of Python ints."""
    c0, c1, c2, c3 = (int(w) & MASK for w in counter)
    k0, k1 = (int(w) & MASK for w in key)
    for _ in range(ROUNDS):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def first_words(n, seed, offset):
    """First output word of the draws of planes 0 .. n-1 under the contract of include/dasac_hip.h (dasac_dropout_planes):
    counter = (plane low, plane high, offset low, offset high), key = (seed low, seed high).  The same rounds as above on numpy
    uint64 lanes (a 32 x 32 bit product fits 64 bits), checked against the scalar form by tests/test_philox_ref_cpu.py."""
    i = np.arange(n, dtype=np.uint64)
    mask = np.uint64(MASK)
    s32 = np.uint64(32)
    c0, c1 = i & mask, i >> s32
    c2 = np.full(n, offset & MASK, np.uint64)
    c3 = np.full(n, (offset >> 32) & MASK, np.uint64)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(ROUNDS):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0.astype(np.int64)


def uniform24(n, seed, offset):
    """k_i = first output word >> 8 (int64 array): the 24-bit integer whose quotient by 2^24 is the plane's uniform."""
    return first_words(n, seed, offset) >> 8
