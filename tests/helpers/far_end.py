"""The far-end inputs of tests/test_far_end_gpu.py and tests/test_far_end_cpu.py: ONE table of seeds, replica ids and counter
positions that every case takes, so that no kernel is compared at the start of a run only (seed below 2^16, counters of a few
hundred, replica ids 0 .. 10).

  SEED_HI      both Philox key words are non-zero and differ; the top bit of the seed (of key word k1) is set
  SEED_CARRY   handles that derive walker keys as seed + i: the carry into the high key word falls inside the batch
  REPLICAS     the largest replica id (2^24 - 1: it shares its counter word with the 8-bit stream tag) and one with every byte used
  lattice sweeps (K1, K7, K8): hs = 2 sweep + colour, sweep0 + n <= 2^31
      end(n)        the call ends exactly at the limit: its last half-sweep is hs = 2^32 - 1
      straddle(n)   the call starts at sweep 2^30 - 3: hs crosses 2^31, the sign bit of an int
  cluster steps, dense and sparse sweeps (K6, K8 clusters, K2, K5): a full uint32 counter, counter0 + n <= 2^32
      end32(n), straddle32(n)
  Potts sweeps (K10, tests/test_potts_far_end_gpu.py): no limit, the counters wrap; potts_positions(n): sweep0 = 2^30 - 3 (hs
      crosses 2^31), 2^31 - 3 (hs wraps through 2^32), 2^32 - 3 (sweep0 + k wraps); its cluster steps: straddle32(n), end32(n)
  multispin coding (K9, tests/helpers/multispin_shapes.py): plane seeds SEED_HI + index, swap seeds SEED_CARRY + s (the carry at
      sample 2), the sweep counter at straddle(n) and end(n), the round counter of its tempering at straddle32(n) and end32(n)
"""
SEED_HI = 0xFEDCBA9876543210
SEED_CARRY = 2 ** 32 - 2
REPLICA_MAX = 2 ** 24 - 1
REPLICA_BYTES = 0xABCDEF
REPLICAS = (REPLICA_MAX, REPLICA_BYTES)

LATTICE_LIMIT = 2 ** 31   # sweep0 + n_sweeps of K1, K7, K8
COUNTER_LIMIT = 2 ** 32   # step0 + n_steps of the cluster steps, sweep0 + n_sweeps of K2 and K5
REPLICA_LIMIT = 2 ** 24


def end(n):
    return LATTICE_LIMIT - n


def straddle(n):
    assert n > 3
    return 2 ** 30 - 3


def end32(n):
    return COUNTER_LIMIT - n


def straddle32(n):
    assert n > 2
    return 2 ** 31 - 2


# Potts sweeps (K10): sweep0 is any uint32, s = sweep0 + k and hs = 2 s + colour are taken modulo 2^32, so a call may begin anywhere
POTTS_HS_SIGN = 2 ** 30 - 3      # hs crosses 2^31, the sign bit of an int, inside a call of 4 sweeps or more
POTTS_HS_WRAP = 2 ** 31 - 3      # hs wraps through 2^32 while sweep0 + k does not
POTTS_SWEEP_WRAP = 2 ** 32 - 3   # sweep0 + k itself wraps through 2^32


def potts_positions(n):
    """(name, sweep0) of the three calls of n sweeps of a Potts case; with n < 4 a call stays on one side of its crossing, at
    counter words with the top bits set (tests/test_potts_far_end_gpu.py).  The Potts cluster steps take counter_positions(n)."""
    assert n >= 1
    return (("hs_sign", POTTS_HS_SIGN), ("hs_wrap", POTTS_HS_WRAP), ("sweep_wrap", POTTS_SWEEP_WRAP))


# The low-half path of the Potts heat bath (potts_site / potts_site6), counted: the model and counters of the two cases whose sites
# decided by lo16 are counted per octet position (tests/test_potts_far_end_cpu.py pins the counts), and the half-sweeps in which one
# octet holds two such sites at J = 0 (tools/potts_lo_pair_search.py finds them): (sweep, colour, global row, octet)
POTTS_FIELD8 = (0.5, -0.5, 0.25, 0.0, -0.25, 0.1, -0.1, 0.3)
POTTS_LO_MODEL = dict(q=8, J=1.0, h=POTTS_FIELD8, T=1.0, seed=SEED_HI, sweep0=2 ** 30 - 1, replica=REPLICA_MAX, n_sweeps=2)
POTTS_LO_SHAPE_3D = (34, 128, 128)   # periodic on every axis
POTTS_LO_SHAPE_2D = (1024, 544)      # periodic
POTTS_LO_PAIR_MODEL = dict(q=8, J=0.0, h=POTTS_FIELD8, T=1.0, seed=SEED_HI, replica=REPLICA_MAX)
POTTS_LO_PAIRS = ((1261, 1, 104, 6), (4915, 1, 114, 4))
POTTS_LO_PAIR_SHAPE_2D = (128, 128)      # periodic
POTTS_LO_PAIR_SHAPE_3D = (8, 16, 128)    # periodic on every axis: the same 128 global rows


def lattice_positions(n):
    """(name, sweep0) of the two calls of n sweeps every lattice case makes, in this order on one handle."""
    return (("straddle", straddle(n)), ("end", end(n)))


def counter_positions(n):
    return (("straddle", straddle32(n)), ("end", end32(n)))
