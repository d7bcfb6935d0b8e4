"""Inputs shared by the scaler / pooling / dB GPU tests (tests/test_scaler_ops_gpu.py) and the CPU pins of their
oracle and bounds (tests/test_oracle_cpu.py): every one is regenerated from a seed."""
import numpy as np

# hlmc_colstats_*: clamp(n / 64, 1, 256) chunks of ceil(n / chunks) rows, one thread per column in blocks of 256.
# n = 1 .. 127: one chunk; 128: two of 64 rows; 129: 65 + 64; 200: three (67 + 67 + 66); 16384: the cap, 256 x 64;
# 16385: 65 rows per chunk, so 252 full ones, one of 5 rows and three empty.
COLSTATS_CASES = [(1, 1), (1, 257), (63, 255), (63, 513), (64, 256), (64, 1), (127, 257), (127, 255), (128, 513),
                  (128, 256), (129, 1), (129, 513), (200, 255), (200, 257), (16384, 256), (16384, 1), (16385, 513),
                  (16385, 255)]
COLSTATS_IDS = [f"n{n}_c{c}" for n, c in COLSTATS_CASES]
CONST_COL, SHIFTED_COL = 5, 6


def colstats_input(n, cols):
    """Columns of different scales and offsets; with room for them, one column constant at 0.1 (not a float32) and
    one with mean 1e4 and standard deviation 1e-2 (a few float32 steps)."""
    rng = np.random.default_rng(100 * n + cols)
    X = (rng.standard_normal((n, cols)) * rng.uniform(0.1, 5, cols) + rng.uniform(-3, 3, cols)).astype(np.float32)
    if cols > SHIFTED_COL:
        X[:, CONST_COL] = 0.1
        X[:, SHIFTED_COL] = (1e4 + 1e-2 * rng.standard_normal(n)).astype(np.float32)
    return X


# StandardScaler.transform: 2040 x 1031 = 2 103 240 elements is past the 8192 x 256 threads of the grid cap, and 1031
# is coprime to that stride, so the column of an element changes from trip to trip of the grid-stride loop.
TRANSFORM_SHAPES = [(300, 513), (2040, 1031), (37, 5, 13)]
TRANSFORM_IDS = ["300x513", "2040x1031_past_grid_cap", "37x5x13_reshape"]


def transform_input(shape):
    n, cols = shape[0], int(np.prod(shape[1:]))
    return colstats_input(n, cols).reshape(shape)


POOL_ROWS = [1, 3, 5, 641]          # 4 rows (waves) per block: 1, 3, 5 and 641 leave a part-filled last block
POOL_COLS = [1, 63, 64, 65, 300]    # one lane, a wave less one, exactly one, one over, several trips
POOL_KINDS = {"db_like": (-30.0, 10.0), "cancelling_mean": (0.0, 1.0)}


def pool_input(rows, cols, kind):
    loc, scale = POOL_KINDS[kind]
    return np.random.default_rng(rows * 1000 + cols).normal(loc, scale, (rows, cols)).astype(np.float32)


# (id, B, F, T, clip of zeros, ref = np.max?, top_db); 3 x 700 001 elements is past the grid cap of 2 097 152 threads
DB_CASES = [("max_top80", 2, 7, 33, 1, True, 80.0), ("max_notop", 2, 7, 33, 1, True, None),
            ("ref1_top80", 2, 7, 33, 0, False, 80.0), ("ref1_notop", 2, 7, 33, 0, False, None),
            ("one_clip_2d", 1, 5, 13, None, True, 80.0),
            ("past_grid_cap", 3, 1, 700001, None, True, 80.0)]
DB_IDS = [c[0] for c in DB_CASES]


def db_input(B, F, T, seed, zero_clip=None):
    """Power values over 18 decades, some below amin = 1e-10, some exactly 0; zero_clip: a clip of zeros only."""
    rng = np.random.default_rng(seed)
    S = np.exp(rng.normal(0.0, 7.0, (B, F, T))).astype(np.float32)
    S[rng.random(S.shape) < 0.05] = 0.0
    S[rng.random(S.shape) < 0.05] = 3e-12
    if zero_clip is not None:
        S[zero_clip] = 0.0
    return S
