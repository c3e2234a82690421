"""Seeded datasets of the wide-domain CI tests (test_gpu_ci_widedom.py) and of their reference fixture
(tests/golden/widedom.ci.gz, make_golden_synth.py widedom): variables with up to 256 states, which
every fast path declines, so each test runs through the byte-column instantiation of the histogram
kernel (ci_kernels.hip).  numpy only; nothing here touches the library under test."""
import numpy as np

# (id, dx, dy, state counts of z_1 .. z_d): one row per table-storage branch of the kernel.  The id
# names the branch; cells = dx * dy * prod(dz).
SHAPES = [
    # <= 16 cells: packed 16-bit per-lane register counters, dx != dy and 1-state variables
    ("packed-5x3", 5, 3, ()),
    ("packed-15x1", 15, 1, ()),
    ("packed-1x16", 1, 16, ()),
    ("packed-2x2|4", 2, 2, (4,)),
    # 17 .. 256 cells: 4 LDS copies per wave
    ("lds4-first-17x1", 17, 1, ()),
    ("lds4-6x3", 6, 3, ()),
    ("lds4-last-16x16", 16, 16, ()),
    # 257 .. 512 cells: 2 copies
    ("lds2-first-43x3|2", 43, 3, (2,)),
    ("lds2-last-32x16", 32, 16, ()),
    # 513 .. 4096 cells: 1 copy; the G^2 terms in chunks of 1024 cells
    ("lds1-first-27x19", 27, 19, ()),
    ("chunk-one-32x32", 32, 32, ()),
    ("chunk-two-41x25", 41, 25, ()),
    ("chunk-two-7x5|11,3", 7, 5, (11, 3)),
    ("lds1-last-64x64", 64, 64, ()),
    # > 4096 cells: one table shared by the workgroup
    ("shared-first-241x17", 241, 17, ()),
    # value 255, tables in global memory
    ("byte255-global-256x256", 256, 256, ()),
    ("byte255-global-256x2|256", 256, 2, (256,)),
    # unequal radices in the z digits
    ("deep-3x21|2,11,5", 3, 21, (2, 11, 5)),
    ("deep-1state-z-6x4|3,1,7,2", 6, 4, (3, 1, 7, 2)),
]
SHAPE_IDS = [s[0] for s in SHAPES]
BYSTANDER_DIM = 5  # one 5-state variable in every batch keeps the 2-bit / bit-sliced paths off
SAMPLE_COUNTS = (1, 255, 1024, 3001)  # scalar loop, fewer samples than threads, dword loop, ragged
SHAPE_SEED = 20260


def columns(dims, n_samples, seed):
    """uint8 [len(dims)][n_samples]: every column a mix of a shared skewed base (so columns depend
    on one another) and its own noise cubed towards the low values (tables far from uniform, empty
    rows and columns in most z-slices of the wide variables); sample v % n_samples of variable v
    holds its top value dims[v] - 1."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, np.int64)
    cols = np.empty((len(dims), n_samples), np.uint8)
    base = (256 * rng.random(n_samples) ** 2).astype(np.int64)
    for v, d in enumerate(dims.tolist()):
        noise = np.minimum(d - 1, (d * rng.random(n_samples) ** 3).astype(np.int64))
        keep = rng.random(n_samples) < 0.4
        cols[v] = np.where(keep, (base * (1 + v % 3) + v) % d, noise)
        cols[v, v % n_samples] = d - 1
    return cols


def shape_layout(shapes=SHAPES):
    """Each shape gets variables of its own, then the bystander: -> (dims int32 [nvars],
    {id: [x, y, z...]}, bystander variable)."""
    dims, items = [], {}
    for sid, dx, dy, dz in shapes:
        v0 = len(dims)
        dims += [dx, dy, *dz]
        items[sid] = list(range(v0, v0 + 2 + len(dz)))
    dims.append(BYSTANDER_DIM)
    return np.asarray(dims, np.int32), items, len(dims) - 1


def shape_dataset(n_samples, shapes=SHAPES):
    dims, items, bystander = shape_layout(shapes)
    return columns(dims, n_samples, SHAPE_SEED + n_samples), dims, items, bystander


def fixture_tests(items):
    """The tests of widedom.ci.gz for one sample count: every shape of at most 5000 cells as laid out,
    with x and y exchanged, and (d >= 2) with the conditioning variables reversed."""
    by_id = {s[0]: s for s in SHAPES}
    tests = []
    for sid, it in items.items():
        _, dx, dy, dz = by_id[sid]
        if dx * dy * int(np.prod(dz, dtype=np.int64)) > 5000:
            continue
        tests.append(list(it))
        tests.append([it[1], it[0]] + it[2:])
        if len(dz) >= 2:
            tests.append(it[:2] + it[2:][::-1])
    return tests


FIXTURE_SAMPLE_COUNTS = (255, 3001)

# ---- the decisions dataset: a forward sample of a seeded network with 2..21 states folded onto
# state counts from {2, 3, 5, 7, 11, 21}, plus a 64-state and a 1-state column set by hand
DECISION_TARGETS = (21, 2, 11, 3, 7, 5, 21, 2, 3, 11, 5, 7, 2, 21, 3, 5, 11, 2, 7, 3, 5, 2)


def decision_dataset(n_samples, tmp_xml):
    """24 variables x n_samples: -> (cols uint8, dims int32).  Variable v < 22 is node v of
    synth.random_network(22, seed=64, dom=(2, 21)) forward-sampled, folded (value % t) onto the
    largest t of {2, 3, 5, 7, 11, 21} within DECISION_TARGETS[v] and its state count; 22: 64 states, a function of variables 0, 6 and
    noise; 23: one state."""
    from fastbn_amd import synth
    synth.random_network(22, seed=64, window=6, parent_probs=(0.5, 0.35, 0.15), dom=(2, 21), path=tmp_xml)
    raw = synth.forward_sample(synth.read_xmlbif(tmp_xml), n_samples, seed=65)
    dom = raw.max(axis=1).astype(np.int64) + 1
    rng = np.random.default_rng(66)
    cols = np.zeros((24, n_samples), np.uint8)
    dims = np.ones(24, np.int32)
    for v in range(22):
        t = max(s for s in (2, 3, 5, 7, 11, 21) if s <= min(DECISION_TARGETS[v], dom[v]))
        cols[v] = raw[v] % t
        dims[v] = t
    cols[22] = (3 * cols[0].astype(np.int64) + 5 * cols[6] + (8 * rng.random(n_samples) ** 2).astype(np.int64)) % 64
    dims[22] = 64
    return cols, dims
