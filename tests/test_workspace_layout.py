"""Every ff_decode*_workspace_bytes query (the fifteen modes' and the greedy decode's with log-probabilities) against tables recorded at the commits BEFORE the refactors of the engine's modes
(the first six columns of TABLE before the decode modes got one size query, decode_workspace_bytes in ff_engine.hip; the other
columns, the "wide" lines and SEQ_TABLE before the engine's Mode became resolved traits): the workspace layout -- the arrays, their order, their sizes -- is part of what a
refactor of the engine must leave alone, and every array is a 256-byte multiple, so a moved or resized one shows in the total.

No GPU: the library loads without one and the queries only do host arithmetic on a hand-filled `lib.Model` whose weight pointers
are null (or, in the "folded" set, non-null dummies: can_fuse_layernorm and layout_decode only test them against null).

`python tests/test_workspace_layout.py` prints the tables of the library it loads (FF_HIP_LIB selects another build); TABLE and
SEQ_TABLE below were printed that way by the parent commit's library and hold no value computed by the code under test.

The "wide" lines have L = 150 edges: five words per row of the loop rule's `visited` array, so that the array is not swallowed by
the 256-byte rounding and one copy (constrain) against the two ping-pong halves (constrained beam) shows in the total.  (A
model's pos_len is not consulted by the queries.)"""
import ctypes as C

from faceformer_amd.hip import engine, lib as L

N, EDGES, F, T, NUM_INPUT = 3, 12, 12, 6, (5, 9, 12)
WIDTH, SAMPLES = 3, 5
FLAGS = {"none": 0, "default": engine.DEFAULT_FLAGS, "retire": engine.DEFAULT_FLAGS | L.FF_RETIRE_FINISHED}
PLANS = {"default": {}, "cw1_ns2": {"chunk_wireframes": 1, "num_streams": 2}, "cs4": {"chunk_seqs": 4}}
WIDE_EDGES = 150
QUERIES = ("greedy", "lp", "beam", "forced", "sample", "constrained", "constrained_ahead", "constrained_exact", "constrained_beam",
           "constrained_beam_ahead", "constrained_sample")
SEQ_QUERIES = ("sequence_sample", "sequence_beam", "sequence_constrained", "sequence_constrained_sample", "sequence_constrained_beam")
SEQ_PLANS = {"default": {}, "cms2_ns2": {"chunk_max_seqs": 2, "num_streams": 2}, "cms1": {"chunk_max_seqs": 1}}   # (N = 3: two / three micro-batches)
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
    """(key, folded, variant, F, flags, plan, edges): every flag set x plan with null weights, the default flags x plan with the
    folded-weight pointers set (x0stat and the pointer-fold arrays enter the layout), one seq2seq line, and the wide shape under
    every plan."""
    for fname, flags in FLAGS.items():
        for pname, plan in PLANS.items():
            yield "plain/%s/%s" % (fname, pname), False, L.FF_PARALLEL, F, flags, plan, EDGES
    for pname, plan in PLANS.items():
        yield "folded/default/%s" % pname, True, L.FF_PARALLEL, F, FLAGS["default"], plan, EDGES
    yield "plain/seq2seq", False, L.FF_SEQ2SEQ, 1, engine.DEFAULT_FLAGS & ~L.FF_DEDUP_PAD_ANCHORS, {}, EDGES
    for pname, plan in PLANS.items():
        yield "wide/default/%s" % pname, False, L.FF_PARALLEL, F, FLAGS["default"], plan, WIDE_EDGES


def seq_cases():
    """(key, folded, flags, plan, edges) of the single-sequence queries (FF_SEQ2SEQ, F = 1): every plan with null and with folded
    weights, and the wide shape under every plan."""
    flags = engine.DEFAULT_FLAGS & ~L.FF_DEDUP_PAD_ANCHORS
    for pname, plan in SEQ_PLANS.items():
        yield "plain/%s" % pname, False, flags, plan, EDGES
        yield "folded/%s" % pname, True, flags, plan, EDGES
        yield "wide/%s" % pname, False, flags, plan, WIDE_EDGES
    yield "plain/none", False, 0, {}, EDGES


def params(variant, f, flags, plan, edges):
    p = L.DecodeParams()
    p.variant, p.N, p.L, p.F, p.T, p.flags, p.sync_every = variant, N, edges, f, T, flags, 4
    for k, v in plan.items():
        setattr(p, k, v)
    return p


def measure(lib):
    out = {}
    ni = (C.c_int * N)(*NUM_INPUT)
    for key, folded, variant, f, flags, plan, edges in cases():
        m, p = model(folded), params(variant, f, flags, plan, edges)
        mp, pp = C.byref(m), C.byref(p)
        out[key] = (lib.ff_decode_workspace_bytes(mp, pp, ni), lib.ff_decode_lp_workspace_bytes(mp, pp, ni),
                    lib.ff_decode_beam_workspace_bytes(mp, pp, ni, WIDTH), lib.ff_decode_forced_workspace_bytes(mp, pp),
                    lib.ff_decode_sample_workspace_bytes(mp, pp, ni, SAMPLES), lib.ff_decode_constrained_workspace_bytes(mp, pp, ni),
                    lib.ff_decode_constrained_ahead_workspace_bytes(mp, pp, ni), lib.ff_decode_constrained_exact_workspace_bytes(mp, pp, ni),
                    lib.ff_decode_constrained_beam_workspace_bytes(mp, pp, ni, WIDTH),
                    lib.ff_decode_constrained_beam_ahead_workspace_bytes(mp, pp, ni, WIDTH),
                    lib.ff_decode_constrained_sample_workspace_bytes(mp, pp, ni, SAMPLES))
    return out


def measure_seq(lib):
    out = {}
    for key, folded, flags, plan, edges in seq_cases():
        m, p = model(folded), params(L.FF_SEQ2SEQ, 1, flags, plan, edges)
        mp, pp = C.byref(m), C.byref(p)
        out[key] = (lib.ff_decode_sequence_sample_workspace_bytes(mp, pp, SAMPLES), lib.ff_decode_sequence_beam_workspace_bytes(mp, pp, WIDTH),
                    lib.ff_decode_sequence_constrained_workspace_bytes(mp, pp),
                    lib.ff_decode_sequence_constrained_sample_workspace_bytes(mp, pp, SAMPLES),
                    lib.ff_decode_sequence_constrained_beam_workspace_bytes(mp, pp, WIDTH))
    return out


# key: (greedy, lp, beam width 3, forced, 5 samples, constrained, constrained_ahead, constrained_exact, constrained beam width 3,
# constrained_beam_ahead width 3, constrained 5 samples) bytes
TABLE = {
    'plain/none/default': (1093888, 1094656, 3040256, 1096192, 4978944, 1100032, 1100032, 1100032, 3047936, 3047936, 4995840),
    'plain/none/cw1_ns2': (808192, 808960, 2183168, 810496, 3549952, 814336, 814336, 814336, 2190848, 2190848, 3566848),
    'plain/none/cs4': (331776, 332544, 541952, 334080, 813568, 337920, 337920, 337920, 549632, 549632, 830464),
    'plain/default/default': (1065728, 1066496, 2955008, 1427968, 4838656, 1070336, 1070336, 1070336, 2961152, 2961152, 4853504),
    'plain/default/cw1_ns2': (1041408, 1042176, 2880512, 1142272, 4715008, 1046016, 1046016, 1046016, 2886400, 2886400, 4728832),
    'plain/default/cs4': (564992, 565760, 1238528, 665856, 1977856, 569600, 569600, 569600, 1244416, 1244416, 1991680),
    'plain/retire/default': (1066496, 1067264, 2956544, 1428736, 4840960, 1071104, 1071104, 1071104, 2962688, 2962688, 4855808),
    'plain/retire/cw1_ns2': (1042176, 1042944, 2882048, 1143040, 4717312, 1046784, 1046784, 1046784, 2887936, 2887936, 4731136),
    'plain/retire/cs4': (565760, 566528, 1240064, 666624, 1980160, 570368, 570368, 570368, 1245952, 1245952, 1993984),
    'folded/default/default': (1148928, 1149696, 3040256, 1503232, 4925696, 1153536, 1153536, 1153536, 3046400, 3046400, 4940544),
    'folded/default/cw1_ns2': (1132800, 1133568, 2973696, 1233920, 4809984, 1137408, 1137408, 1137408, 2979584, 2979584, 4823808),
    'folded/default/cs4': (697600, 698368, 1538048, 807168, 2279168, 702208, 702208, 702208, 1543936, 1543936, 2292992),
    'plain/seq2seq': (233472, 233728, 451072, 234240, 668160, 235264, 235264, 235264, 452352, 452352, 670208),
    'wide/default/default': (2138880, 2139648, 4054784, 2507776, 5964800, 2148352, 2148352, 2148352, 4076544, 4076544, 6002688),
    'wide/default/cw1_ns2': (2114560, 2115328, 3980288, 2215424, 5841408, 2123520, 2123520, 2123520, 4000512, 4000512, 5876736),
    'wide/default/cs4': (1627136, 1627904, 2300160, 1728000, 3040512, 1636096, 1636096, 1636096, 2320384, 2320384, 3075840),
}

# key: (5 samples, beam width 3, constrained, constrained 5 samples, constrained beam width 3) bytes of the ff_decode_sequence_* queries
SEQ_TABLE = {
    'plain/default': (668160, 451072, 235264, 670208, 452608),
    'folded/default': (742656, 525568, 309504, 744704, 527104),
    'wide/default': (1736448, 1515776, 1297152, 1741056, 1518848),
    'plain/cms2_ns2': (549376, 379648, 259328, 551424, 381184),
    'folded/cms2_ns2': (640256, 470528, 341760, 642304, 472064),
    'wide/cms2_ns2': (1614848, 1443072, 1321472, 1619456, 1446144),
    'plain/cms1': (430080, 307968, 187648, 432128, 309504),
    'folded/cms1': (520960, 398848, 278272, 523008, 400384),
    'wide/cms1': (1492736, 1369600, 1248256, 1497344, 1372672),
    'plain/none': (529920, 368128, 207616, 531968, 369664),
}


def test_workspace_bytes_are_the_recorded_ones(hip_lib):
    for got, table, names in ((measure(hip_lib), TABLE, QUERIES), (measure_seq(hip_lib), SEQ_TABLE, SEQ_QUERIES)):
        assert sorted(got) == sorted(table)
        for key in table:
            assert len(got[key]) == len(names) and all(v > 0 for v in got[key]), key
            assert got[key] == table[key], (key, dict(zip(names, got[key])), dict(zip(names, table[key])))


def test_queries_keep_their_argument_checks(hip_lib):
    m, p = model(False), L.DecodeParams()
    p.variant, p.N, p.L, p.F, p.T, p.flags = L.FF_PARALLEL, N, EDGES, F, T, engine.DEFAULT_FLAGS
    mp, pp, ni = C.byref(m), C.byref(p), (C.c_int * N)(*NUM_INPUT)
    sq = params(L.FF_SEQ2SEQ, 1, engine.DEFAULT_FLAGS & ~L.FF_DEDUP_PAD_ANCHORS, {}, EDGES)
    sp = C.byref(sq)
    h = hip_lib
    by_width = [lambda a, b, w: h.ff_decode_beam_workspace_bytes(a, b, ni, w), lambda a, b, w: h.ff_decode_constrained_beam_workspace_bytes(a, b, ni, w),
                lambda a, b, w: h.ff_decode_constrained_beam_ahead_workspace_bytes(a, b, ni, w)]
    by_samples = [lambda a, b, r: h.ff_decode_sample_workspace_bytes(a, b, ni, r),
                  lambda a, b, r: h.ff_decode_constrained_sample_workspace_bytes(a, b, ni, r)]
    seq_by_width = [h.ff_decode_sequence_beam_workspace_bytes, h.ff_decode_sequence_constrained_beam_workspace_bytes]
    seq_by_samples = [h.ff_decode_sequence_sample_workspace_bytes, h.ff_decode_sequence_constrained_sample_workspace_bytes]
    for qs, par in ((by_width, pp), (seq_by_width, sp)):
        for q in qs:
            assert [q(mp, par, w) == 0 for w in (0, 1, 8, 9)] == [True, False, False, True]
    for qs, par in ((by_samples, pp), (seq_by_samples, sp)):
        for q in qs:
            assert [q(mp, par, r) == 0 for r in (0, 1, 64, 65)] == [True, False, False, True]
    queries = [lambda a, b: h.ff_decode_workspace_bytes(a, b, ni), lambda a, b: h.ff_decode_lp_workspace_bytes(a, b, ni),
               h.ff_decode_forced_workspace_bytes, lambda a, b: h.ff_decode_constrained_workspace_bytes(a, b, ni),
               lambda a, b: h.ff_decode_constrained_ahead_workspace_bytes(a, b, ni),
               lambda a, b: h.ff_decode_constrained_exact_workspace_bytes(a, b, ni)]
    queries += [lambda a, b, q=q: q(a, b, WIDTH) for q in by_width] + [lambda a, b, q=q: q(a, b, SAMPLES) for q in by_samples]
    seq_queries = [h.ff_decode_sequence_constrained_workspace_bytes]
    seq_queries += [lambda a, b, q=q: q(a, b, WIDTH) for q in seq_by_width] + [lambda a, b, q=q: q(a, b, SAMPLES) for q in seq_by_samples]
    entries = [k for k in L.SIGNATURES if k.startswith("ff_decode") and k.endswith("_workspace_bytes")]
    assert len(queries) + len(seq_queries) == len(QUERIES) + len(SEQ_QUERIES) == len(entries)   # (every such entry of the library)
    for qs, par in ((queries, pp), (seq_queries, sp)):
        for q in qs:
            assert q(mp, par) > 0
            assert q(None, par) == 0 and q(mp, None) == 0
            for field in ("N", "F", "T"):
                bad = L.DecodeParams()
                C.memmove(C.byref(bad), par, C.sizeof(bad))
                setattr(bad, field, 0)
                assert q(mp, C.byref(bad)) == 0, field
    # a sequence query is for FF_SEQ2SEQ with F = 1 only: 0 for a parallel-variant struct and for any other F
    for q in seq_queries:
        assert q(mp, pp) == 0
        for variant, f in ((L.FF_PARALLEL, 1), (L.FF_SEQ2SEQ, 2), (L.FF_SEQ2SEQ, F)):
            bad = params(variant, f, sq.flags, {}, EDGES)
            assert q(mp, C.byref(bad)) == 0, (variant, f)


if __name__ == "__main__":
    for name, table in (("TABLE", measure(L.load())), ("SEQ_TABLE", measure_seq(L.load()))):
        print("%s = {" % name)
        for key, vals in table.items():
            print("    %r: %r," % (key, vals))
        print("}")
