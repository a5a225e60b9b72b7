"""The six ff_decode*_workspace_bytes queries against a table recorded at the commit BEFORE the decode modes got one size query
(decode_workspace_bytes, ff_engine.hip): the workspace layout -- the arrays, their order, their sizes -- is part of what a
refactor of the engine must leave alone, and every array is a 256-byte multiple, so a moved or resized one shows in the total.

No GPU: the library loads without one and the queries only do host arithmetic on a hand-filled `lib.Model` whose weight pointers
are null (or, in the "folded" set, non-null dummies: can_fuse_layernorm and layout_decode only test them against null).

`python tests/test_workspace_layout.py` prints the table of the library it loads (FF_HIP_LIB selects another build); TABLE below
was printed that way by the parent commit's library and holds no value computed by the code under test."""
import ctypes as C

from faceformer_amd.hip import engine, lib as L

N, EDGES, F, T, NUM_INPUT = 3, 12, 12, 6, (5, 9, 12)
WIDTH, SAMPLES = 3, 5
FLAGS = {"none": 0, "default": engine.DEFAULT_FLAGS, "retire": engine.DEFAULT_FLAGS | L.FF_RETIRE_FINISHED}
PLANS = {"default": {}, "cw1_ns2": {"chunk_wireframes": 1, "num_streams": 2}, "cs4": {"chunk_seqs": 4}}
QUERIES = ("greedy", "lp", "beam", "forced", "sample", "constrained")
DUMMY = 0x1000   # a non-null address the queries never read through


def model(folded):
    m = L.Model()
    m.E, m.H, m.FF, m.num_enc_layers, m.num_dec_layers, m.in_dim, m.num_token = 128, 2, 256, 1, 2, 4, 4
    m.pos_len, m.qpos_len, m.ln_eps = 64, 64, 1e-5
    if folded:
        m.proj_fold_w = m.proj_fold_b = DUMMY
        for i in range(m.num_dec_layers):
            for f in ("ln1_w", "ln1_b", "ln1_pos", "ln2_w", "ln2_b", "ln2_pos", "ln3_w", "ln3_b"):
                setattr(m.dec[i], f, DUMMY)
    return m


def cases():
    """(key, folded, variant, F, flags, plan): every flag set x plan with null weights, the default flags x plan with the
    folded-weight pointers set (x0stat and the pointer-fold arrays enter the layout), and one seq2seq line."""
    for fname, flags in FLAGS.items():
        for pname, plan in PLANS.items():
            yield "plain/%s/%s" % (fname, pname), False, L.FF_PARALLEL, F, flags, plan
    for pname, plan in PLANS.items():
        yield "folded/default/%s" % pname, True, L.FF_PARALLEL, F, FLAGS["default"], plan
    yield "plain/seq2seq", False, L.FF_SEQ2SEQ, 1, engine.DEFAULT_FLAGS & ~L.FF_DEDUP_PAD_ANCHORS, {}


def measure(lib):
    out = {}
    ni = (C.c_int * N)(*NUM_INPUT)
    for key, folded, variant, f, flags, plan in cases():
        m, p = model(folded), L.DecodeParams()
        p.variant, p.N, p.L, p.F, p.T, p.flags, p.sync_every = variant, N, EDGES, f, T, flags, 4
        for k, v in plan.items():
            setattr(p, k, v)
        mp, pp = C.byref(m), C.byref(p)
        out[key] = (lib.ff_decode_workspace_bytes(mp, pp, ni), lib.ff_decode_lp_workspace_bytes(mp, pp, ni),
                    lib.ff_decode_beam_workspace_bytes(mp, pp, ni, WIDTH), lib.ff_decode_forced_workspace_bytes(mp, pp),
                    lib.ff_decode_sample_workspace_bytes(mp, pp, ni, SAMPLES), lib.ff_decode_constrained_workspace_bytes(mp, pp, ni))
    return out


# key: (greedy, lp, beam width 3, forced, 5 samples, constrained) bytes
TABLE = {
    'plain/none/default': (1093888, 1094656, 3040256, 1096192, 4978944, 1100032),
    'plain/none/cw1_ns2': (808192, 808960, 2183168, 810496, 3549952, 814336),
    'plain/none/cs4': (331776, 332544, 541952, 334080, 813568, 337920),
    'plain/default/default': (1065728, 1066496, 2955008, 1427968, 4838656, 1070336),
    'plain/default/cw1_ns2': (1041408, 1042176, 2880512, 1142272, 4715008, 1046016),
    'plain/default/cs4': (564992, 565760, 1238528, 665856, 1977856, 569600),
    'plain/retire/default': (1066496, 1067264, 2956544, 1428736, 4840960, 1071104),
    'plain/retire/cw1_ns2': (1042176, 1042944, 2882048, 1143040, 4717312, 1046784),
    'plain/retire/cs4': (565760, 566528, 1240064, 666624, 1980160, 570368),
    'folded/default/default': (1148928, 1149696, 3040256, 1503232, 4925696, 1153536),
    'folded/default/cw1_ns2': (1132800, 1133568, 2973696, 1233920, 4809984, 1137408),
    'folded/default/cs4': (697600, 698368, 1538048, 807168, 2279168, 702208),
    'plain/seq2seq': (233472, 233728, 451072, 234240, 668160, 235264),
}


def test_workspace_bytes_are_the_recorded_ones(hip_lib):
    got = measure(hip_lib)
    assert sorted(got) == sorted(TABLE)
    for key in TABLE:
        assert all(v > 0 for v in got[key]), key
        assert got[key] == TABLE[key], (key, dict(zip(QUERIES, got[key])), dict(zip(QUERIES, TABLE[key])))


def test_queries_keep_their_argument_checks(hip_lib):
    m, p = model(False), L.DecodeParams()
    p.variant, p.N, p.L, p.F, p.T, p.flags = L.FF_PARALLEL, N, EDGES, F, T, engine.DEFAULT_FLAGS
    mp, pp, ni = C.byref(m), C.byref(p), (C.c_int * N)(*NUM_INPUT)
    for w in (0, 9):
        assert hip_lib.ff_decode_beam_workspace_bytes(mp, pp, ni, w) == 0
    for r in (0, 65):
        assert hip_lib.ff_decode_sample_workspace_bytes(mp, pp, ni, r) == 0
    assert hip_lib.ff_decode_beam_workspace_bytes(mp, pp, ni, 8) > 0 and hip_lib.ff_decode_sample_workspace_bytes(mp, pp, ni, 64) > 0
    queries = [lambda a, b: hip_lib.ff_decode_workspace_bytes(a, b, ni), lambda a, b: hip_lib.ff_decode_lp_workspace_bytes(a, b, ni),
               lambda a, b: hip_lib.ff_decode_beam_workspace_bytes(a, b, ni, WIDTH), hip_lib.ff_decode_forced_workspace_bytes,
               lambda a, b: hip_lib.ff_decode_sample_workspace_bytes(a, b, ni, SAMPLES),
               lambda a, b: hip_lib.ff_decode_constrained_workspace_bytes(a, b, ni)]
    for q in queries:
        assert q(None, pp) == 0 and q(mp, None) == 0
        for field in ("N", "F", "T"):
            bad = L.DecodeParams()
            C.memmove(C.byref(bad), pp, C.sizeof(bad))
            setattr(bad, field, 0)
            assert q(mp, C.byref(bad)) == 0, field


if __name__ == "__main__":
    print("TABLE = {")
    for key, vals in measure(L.load()).items():
        print("    %r: %r," % (key, vals))
    print("}")
