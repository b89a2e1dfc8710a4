"""Every refusal of the C ABI's row-operand wrappers, pinned on the CPU: each call below returns before any HIP call.

One row per entry point: the argument names in ABI order, a call that WOULD launch (pointers are the aligned non-null dummy 16,
never dereferenced), and the cases -- one argument changed, the status expected.  The statuses are the header's (0 OK, -1 invalid
argument, -2 unsupported) as the library answered before its host wrappers were given one validation layer; the table is what keeps
them where they were.  Not in the table, because the library accepts them and goes on to launch: a misaligned operand that a kernel
reads with scalar loads (the bias of rdetr_linear_*, b1 / b2 of the MLP heads, gamma / beta of rdetr_linear_ln_k256_bf16), and a
misaligned or off-grid operand of the inference add_layernorm entries and of the two token-layout entries, which select the
generic kernel instead of refusing.
"""
import ctypes

import pytest

from relation_detr_amd import _lib

ONE = ctypes.c_void_p(16)              # aligned, non-null
P8 = ctypes.c_void_p(8)                # on the 8-byte grid only
P4 = ctypes.c_void_p(4)
P17 = ctypes.c_void_p(17)
P2 = ctypes.c_void_p(2)

SHAPES = (ctypes.c_int64 * 8)(64, 96, 32, 48, 16, 24, 8, 12)
STARTS = (ctypes.c_int64 * 4)(0, 6144, 7680, 8064)
LEVEL_SRC = (ctypes.c_void_p * 2)(16, 16)
LEVEL_SRC_HOLE = (ctypes.c_void_p * 2)(16, None)
LEVEL_PIXELS = (ctypes.c_int * 2)(64, 16)
LEVEL_PIXELS_NEG = (ctypes.c_int * 2)(64, -1)
LEVEL_PIXELS_ZERO = (ctypes.c_int * 2)(0, 0)


def each(names, value, status):
    return [({n: value}, status) for n in names.split()]


LINEAR = ("x ldx w bias M N relu out ldo stream", dict(x=ONE, ldx=256, w=ONE, bias=ONE, M=4, N=256, relu=0, out=ONE, ldo=256, stream=None))
LINEAR_HM = ("x ldx w bias row_mask B S out stream", dict(x=ONE, ldx=256, w=ONE, bias=None, row_mask=None, B=1, S=4, out=ONE, stream=None))
LINEAR_LN = ("x ldx packed bias res ldr gamma beta eps M out ldo stream",
             dict(x=ONE, ldx=256, packed=ONE, bias=None, res=ONE, ldr=256, gamma=ONE, beta=ONE, eps=1e-5, M=4, out=ONE, ldo=256, stream=None))
LINEAR_LN_ROWS = ("x ldx packed bias res ldr gamma beta eps pos ldp M out ldo out_pos ldop stream",
                  dict(x=ONE, ldx=256, packed=ONE, bias=None, res=ONE, ldr=256, gamma=ONE, beta=ONE, eps=1e-5, pos=None, ldp=0, M=4, out=ONE,
                       ldo=256, out_pos=None, ldop=0, stream=None))
WITH_POS = dict(pos=ONE, ldp=256, out_pos=ONE, ldop=256)
BOX = ("xa lda xb ldb pw1 b1 pw2 b2 w3 b3 ref logit eps M out_a out_b stream",
       dict(xa=ONE, lda=256, xb=None, ldb=0, pw1=ONE, b1=ONE, pw2=ONE, b2=ONE, w3=ONE, b3=ONE, ref=ONE, logit=0, eps=1e-3, M=4, out_a=ONE,
            out_b=None, stream=None))
BOX_CLS = ("xa lda xb ldb pw1 b1 pw2 b2 w3 b3 ref logit eps pwc bc C M out_a out_b out_cls ldc stream",
           dict(BOX[1], pwc=ONE, bc=ONE, C=91, out_cls=ONE, ldc=91))
WITH_B = dict(xb=ONE, ldb=256, out_b=ONE)
QPOS = ("emb lde query ldq pw1a pw1b b1 pw2 b2 pv1 c1 pv2 c2 M out_pos out_qpp stream",
        dict(emb=ONE, lde=512, query=ONE, ldq=256, pw1a=ONE, pw1b=ONE, b1=ONE, pw2=ONE, b2=ONE, pv1=None, c1=None, pv2=None, c2=None, M=4,
             out_pos=ONE, out_qpp=ONE, stream=None))
QPOS_IN = ("emb lde query ldq pw1a pw1b b1 pw2 b2 pv1 c1 pv2 c2 pwq pwk pwv bias M out_pos out_qpp out_qk ldqk out_v ldv stream",
           dict(QPOS[1], pwq=ONE, pwk=ONE, pwv=ONE, bias=ONE, out_qk=ONE, ldqk=512, out_v=ONE, ldv=256))
SCALED = dict(pv1=ONE, c1=ONE, pv2=ONE, c2=ONE)
ENC_PROJ = ("x ldx xq ldq pwv bv pwq bq row_mask B S q_cols out_hm out_q stream",
            dict(x=ONE, ldx=256, xq=ONE, ldq=256, pwv=ONE, bv=None, pwq=ONE, bq=None, row_mask=None, B=1, S=4, q_cols=384, out_hm=ONE, out_q=ONE,
                 stream=None))
LN_STRIDED = ("x r gamma beta rows C ldx ldr ldo eps out stream",
              dict(x=ONE, r=None, gamma=ONE, beta=ONE, rows=4, C=256, ldx=256, ldr=0, ldo=256, eps=1e-5, out=ONE, stream=None))
LN_POS = ("x r gamma beta pos rows C ldx ldr ldo ldp ldo2 eps out out2 stream",
          dict(x=ONE, r=None, gamma=ONE, beta=ONE, pos=ONE, rows=4, C=256, ldx=256, ldr=0, ldo=256, ldp=256, ldo2=256, eps=1e-5, out=ONE,
               out2=ONE, stream=None))
LN_TRAIN = ("x r gamma beta rows C ldx ldr ldo eps out stats stream", dict(LN_STRIDED[1], stats=ONE))
LN_BWD = ("dy lddy x ldx r ldr gamma stats rows C ws wsb dx dgamma dbeta stream",
          dict(dy=ONE, lddy=256, x=ONE, ldx=256, r=None, ldr=0, gamma=ONE, stats=ONE, rows=4, C=256, ws=None, wsb=0, dx=ONE, dgamma=None,
               dbeta=None, stream=None))
LN_TRAIN_MIXED = ("x xb ldx r rb ldr gamma beta rows C eps out ldo stats stream",
                  dict(x=ONE, xb=1, ldx=256, r=None, rb=0, ldr=0, gamma=ONE, beta=ONE, rows=4, C=256, eps=1e-5, out=ONE, ldo=256, stats=ONE,
                       stream=None))
LN_BWD_MIXED = ("dy lddy x xb ldx r rb ldr gamma stats rows C ws wsb dx dxb dgamma dbeta stream",
                dict(dy=ONE, lddy=256, x=ONE, xb=1, ldx=256, r=None, rb=0, ldr=0, gamma=ONE, stats=ONE, rows=4, C=256, ws=None, wsb=0, dx=None,
                     dxb=ONE, dgamma=None, dbeta=None, stream=None))
PARAM_GRADS = dict(dgamma=ONE, dbeta=ONE, ws=ONE, wsb=4096)
TOKENS = ("src add_vec is_bf16 B C P ois ld_out out stream",
          dict(src=ONE, add_vec=None, is_bf16=1, B=1, C=256, P=64, ois=16384, ld_out=256, out=ONE, stream=None))
TOKENS_LEVELS = ("level_src level_vec level_pixels L is_bf16 B C ois ld_out out stream",
                 dict(level_src=LEVEL_SRC, level_vec=None, level_pixels=LEVEL_PIXELS, L=2, is_bf16=1, B=1, C=256, ois=20480, ld_out=256, out=ONE,
                      stream=None))
FFN = ("x ldx packed b1 b2 M F out ldo stream", dict(x=ONE, ldx=256, packed=ONE, b1=ONE, b2=ONE, M=4, F=2048, out=ONE, ldo=256, stream=None))
FFN_LN = ("x ldx packed b1 b2 gamma beta eps pos ldp M F out ldo out2 ldo2 stream",
          dict(FFN[1], gamma=ONE, beta=ONE, eps=1e-5, pos=None, ldp=0, out2=None, ldo2=0))
FFN_TRAIN = ("x ldx packed b1 b2 M F out ldo hid ldh stream", dict(FFN[1], hid=ONE, ldh=2048))
FFN_TRAIN_XF32 = ("x ldx packed b1 b2 M F out ldo hid ldh xlp ldxl stream", dict(FFN_TRAIN[1], xlp=ONE, ldxl=256))
FFN_BWD = ("dy lddy packed_t hid ldh M F dh ldd dx lddx stream",
           dict(dy=ONE, lddy=256, packed_t=ONE, hid=ONE, ldh=2048, M=4, F=2048, dh=ONE, ldd=2048, dx=ONE, lddx=256, stream=None))
FFN_PACK = ("w1 w2 F packed stream", dict(w1=ONE, w2=ONE, F=2048, packed=ONE, stream=None))
FFN_PACK_F32 = ("w1 rs1 cs1 w2 rs2 cs2 b1 b2 F packed biases stream",
                dict(w1=ONE, rs1=256, cs1=1, w2=ONE, rs2=2048, cs2=1, b1=None, b2=None, F=2048, packed=ONE, biases=None, stream=None))
RESIDENT = ("value shapes starts loc attn B S H D L Nq P out stream",
            dict(value=ONE, shapes=SHAPES, starts=STARTS, loc=ONE, attn=ONE, B=1, S=8160, H=8, D=32, L=4, Nq=8160, P=4, out=ONE, stream=None))
RESIDENT_FUSED = ("value shapes starts offs ld_offs logits ld_logits ref ref_dim B S H D L Nq P out stream",
                  dict(value=ONE, shapes=SHAPES, starts=STARTS, offs=ONE, ld_offs=0, logits=ONE, ld_logits=0, ref=ONE, ref_dim=2, B=1, S=8160,
                       H=8, D=32, L=4, Nq=8160, P=4, out=ONE, stream=None))

FFN_ROW_CASES = ([({"M": 0}, 0), ({"M": -1}, -1), ({"F": 0}, -1), ({"F": 100}, -2), ({"F": 4160, "ldh": 4160}, -2), ({"ldx": 255}, -1), ({"ldo": 255}, -1),
                  ({"ldx": 260}, -2), ({"ldo": 260}, -2)]
                 + each("x packed b1 b2 out", None, -1) + each("x packed out", P8, -2))
FFN_BWD_CASES = ([({"M": 0}, 0), ({"M": -1}, -1), ({"F": 100}, -2), ({"lddy": 255}, -1), ({"lddx": 255}, -1), ({"ldh": 2047}, -1), ({"ldd": 2047}, -1),
                  ({"lddy": 260}, -2), ({"ldh": 2052}, -2), ({"ldd": 2052}, -2), ({"M": 1 << 20}, -2)]
                 + each("dy packed_t hid dh dx", None, -1) + each("dy packed_t hid dh dx", P8, -2))


def ln_train_cases(off_grid):
    return ([({"rows": 0}, 0), ({"rows": -1}, -1), ({"C": 0}, -1), ({"C": 128}, -2), ({"ldx": 255}, -1), ({"ldo": 255}, -1),
             ({"r": ONE, "ldr": 255}, -1), ({"ldx": off_grid}, -2), ({"ldo": off_grid}, -2), ({"r": ONE, "ldr": off_grid}, -2),
             ({"r": P8, "ldr": 256}, -2), ({"stats": P4}, -2)]
            + each("x gamma beta out stats", None, -1) + each("x gamma beta out", P8, -2))


def ln_bwd_cases(off_grid):
    return ([({"rows": 0}, 0), ({"rows": -1}, -1), ({"C": 128}, -2), ({"lddy": 255}, -1), ({"ldx": 255}, -1), ({"r": ONE, "ldr": 255}, -1),
             ({"wsb": -1}, -1), ({"dgamma": ONE}, -1), ({"dbeta": ONE}, -1), (dict(PARAM_GRADS, ws=None), -1), (dict(PARAM_GRADS, wsb=100), -1),
             (dict(PARAM_GRADS, ws=P8), -2), ({"lddy": off_grid}, -2), ({"ldx": off_grid}, -2), ({"r": ONE, "ldr": off_grid}, -2),
             ({"r": P8, "ldr": 256}, -2), ({"stats": P4}, -2)]
            + each("dy x gamma stats dx", None, -1) + each("dy x gamma dx", P8, -2))


LN_INFER_CASES = [({"rows": 0}, 0), ({"rows": -1}, -1), ({"C": 0}, -1), ({"C": 8193, "ldx": 8193, "ldo": 8193}, -1), ({"ldx": 255}, -1),
                  ({"ldo": 255}, -1), ({"r": ONE, "ldr": 255}, -1)] + each("x gamma beta out", None, -1)

TABLE = {
    "rdetr_linear_k256_bf16": LINEAR + (
        [({"M": 0}, 0), ({"M": -1}, -1), ({"N": 0}, -1), ({"N": 48}, -2), ({"ldx": 255}, -1), ({"ldo": 255}, -1), ({"ldx": 260}, -2),
         ({"ldo": 260}, -2)] + each("x w out", None, -1) + each("x w out", P8, -2),),
    "rdetr_linear_k256_hm_bf16": LINEAR_HM + (
        [({"B": 0}, 0), ({"S": 0}, 0), ({"B": -1}, -1), ({"S": -1}, -1), ({"ldx": 255}, -1), ({"ldx": 260}, -2), ({"B": 65536, "S": 65536}, -2)]
        + each("x w out", None, -1) + each("x w out", P8, -2),),
    "rdetr_linear_pack_k256_bf16": ("w packed stream", dict(w=ONE, packed=ONE, stream=None), each("w packed", None, -1) + each("w packed", P8, -2)),
    "rdetr_linear_ln_k256_bf16": LINEAR_LN + (
        [({"M": 0}, 0), ({"M": -1}, -1)] + each("ldx ldr ldo", 255, -1) + each("ldx ldr ldo", 260, -2)
        + each("x packed res gamma beta out", None, -1) + each("x packed res out", P8, -2),),
    "rdetr_linear_ln_rows_bf16": LINEAR_LN_ROWS + (
        [({"M": 0}, 0), ({"M": -1}, -1)] + each("ldx ldr ldo", 255, -1) + each("ldx ldr ldo", 260, -2)
        + each("x packed res gamma beta out", None, -1) + each("x packed bias res gamma beta out", P8, -2)
        + [(dict(WITH_POS, **c), s) for c, s in each("ldp ldop", 255, -1) + each("ldp ldop", 260, -2) + each("pos out_pos", P8, -2)
           + [({"out_pos": None}, -1)]],),
    "rdetr_box_head_k256_bf16": BOX + (
        [({"M": 0}, 0), ({"M": -1}, -1), ({"lda": 255}, -1), ({"lda": 260}, -2)] + each("xa pw1 b1 pw2 b2 w3 b3 ref out_a", None, -1)
        + each("xa pw1 pw2 w3 ref out_a", P8, -2)
        + [(dict(WITH_B, **c), s) for c, s in [({"ldb": 255}, -1), ({"ldb": 260}, -2), ({"out_b": None}, -1), ({"xb": P8}, -2), ({"out_b": P8}, -2)]],),
    "rdetr_box_head_cls_k256_bf16": BOX_CLS + (
        [({"M": 0}, 0), ({"M": -1}, -1), ({"lda": 255}, -1), ({"lda": 260}, -2), ({"C": 0}, -1), ({"C": 257, "ldc": 257}, -2), ({"ldc": 90}, -1)]
        + each("xa pw1 b1 pw2 b2 w3 b3 ref out_a pwc bc out_cls", None, -1) + each("xa pw1 pw2 w3 ref out_a pwc", P8, -2)
        + each("bc out_cls", P17, -2)
        + [(dict(WITH_B, **c), s) for c, s in [({"ldb": 255}, -1), ({"ldb": 260}, -2), ({"out_b": None}, -1), ({"xb": P8}, -2), ({"out_b": P8}, -2)]],),
    "rdetr_query_pos_k256_bf16": QPOS + (
        [({"M": 0}, 0), ({"M": -1}, -1), ({"lde": 511}, -1), ({"ldq": 255}, -1), ({"lde": 516}, -2), ({"ldq": 260}, -2), ({"pv1": ONE}, -1),
         (dict(SCALED, c2=None), -1), (dict(SCALED, pv1=P8), -2), (dict(SCALED, pv2=P8), -2)]
        + each("emb query pw1a pw1b b1 pw2 b2 out_pos out_qpp", None, -1) + each("emb query pw1a pw1b pw2 out_pos out_qpp", P8, -2),),
    "rdetr_query_pos_inproj_k256_bf16": QPOS_IN + (
        [({"M": 0}, 0), ({"M": -1}, -1), ({"lde": 511}, -1), ({"ldq": 255}, -1), ({"ldqk": 511}, -1), ({"ldv": 255}, -1), ({"lde": 516}, -2),
         ({"ldq": 260}, -2), ({"ldqk": 516}, -2), ({"ldv": 260}, -2), ({"pv1": ONE}, -1), (dict(SCALED, pv1=P8), -2)]
        + each("emb query pw1a pw1b b1 pw2 b2 out_pos out_qpp pwq pwk pwv bias out_qk out_v", None, -1)
        + each("emb query pw1a pw1b pw2 out_pos out_qpp pwq pwk pwv out_qk out_v", P8, -2),),
    "rdetr_encoder_proj_k256_bf16": ENC_PROJ + (
        [({"B": 0}, 0), ({"S": 0}, 0), ({"B": -1}, -1), ({"S": -1}, -1), ({"q_cols": 256}, -2), ({"q_cols": 512}, -2), ({"ldx": 255}, -1),
         ({"ldq": 255}, -1), ({"ldx": 260}, -2), ({"ldq": 260}, -2), ({"q_cols": 256, "ldx": 255}, -1)]
        + each("x xq pwv pwq out_hm out_q", None, -1) + each("x xq pwv pwq out_hm out_q", P8, -2),),
    "rdetr_add_layernorm_strided_f32": LN_STRIDED + (LN_INFER_CASES,),
    "rdetr_add_layernorm_strided_bf16": LN_STRIDED + (LN_INFER_CASES,),
    "rdetr_add_layernorm_pos_f32": LN_POS + (LN_INFER_CASES + each("pos out2", None, -1) + each("ldp ldo2", 255, -1),),
    "rdetr_add_layernorm_pos_bf16": LN_POS + (LN_INFER_CASES + each("pos out2", None, -1) + each("ldp ldo2", 255, -1),),
    "rdetr_add_layernorm_train_f32": LN_TRAIN + (ln_train_cases(258),),
    "rdetr_add_layernorm_train_bf16": LN_TRAIN + (ln_train_cases(260),),
    "rdetr_add_layernorm_backward_f32": LN_BWD + (ln_bwd_cases(258),),
    "rdetr_add_layernorm_backward_bf16": LN_BWD + (ln_bwd_cases(260),),
    "rdetr_add_layernorm_train_mixed": LN_TRAIN_MIXED + (
        [({"rows": 0}, 0), ({"rows": -1}, -1), ({"C": 128}, -2), ({"ldx": 255}, -1), ({"ldo": 255}, -1), ({"r": ONE, "ldr": 255}, -1),
         ({"ldx": 260}, -2), ({"xb": 0, "ldx": 258}, -2), ({"ldo": 258}, -2), ({"r": ONE, "rb": 1, "ldr": 260}, -2), ({"r": ONE, "ldr": 258}, -2),
         ({"r": P8, "ldr": 256}, -2), ({"stats": P4}, -2)]
        + each("x gamma beta out stats", None, -1) + each("x gamma beta out", P8, -2),),
    "rdetr_add_layernorm_backward_mixed": LN_BWD_MIXED + (
        [({"rows": 0}, 0), ({"rows": -1}, -1), ({"C": 128}, -2), ({"lddy": 255}, -1), ({"ldx": 255}, -1), ({"r": ONE, "ldr": 255}, -1),
         ({"dxb": None}, -1), ({"xb": 0}, -1), ({"r": ONE, "ldr": 256}, -1), ({"dgamma": ONE}, -1), (dict(PARAM_GRADS, ws=None), -1),
         (dict(PARAM_GRADS, wsb=100), -1), (dict(PARAM_GRADS, ws=P8), -2), ({"lddy": 258}, -2), ({"ldx": 260}, -2),
         ({"xb": 0, "dx": ONE, "ldx": 258}, -2), ({"r": P8, "rb": 1, "ldr": 256}, -2), ({"r": ONE, "rb": 1, "ldr": 260}, -2), ({"stats": P4}, -2),
         ({"dxb": P8}, -2), ({"dx": P8}, -2)]
        + each("dy x gamma stats", None, -1) + each("dy x gamma", P8, -2),),
    "rdetr_nchw_to_tokens": TOKENS + (
        [({"B": 0}, 0), ({"P": 0}, 0), ({"B": -1}, -1), ({"C": 0}, -1), ({"ld_out": 255}, -1), ({"ois": -1}, -1), ({"B": 65536}, -2)]
        + each("src out", None, -1),),
    "rdetr_nchw_levels_to_tokens": TOKENS_LEVELS + (
        [({"B": 0}, 0), ({"level_pixels": LEVEL_PIXELS_ZERO}, 0), ({"L": 0}, -1), ({"B": -1}, -1), ({"C": 0}, -1), ({"ld_out": 255}, -1),
         ({"level_pixels": LEVEL_PIXELS_NEG}, -1), ({"level_src": LEVEL_SRC_HOLE}, -1), ({"L": 9}, -2), ({"B": 65536}, -2), ({"is_bf16": 2}, -2)]
        + each("level_src level_pixels out", None, -1),),
    "rdetr_ffn_k256_pack_bf16": FFN_PACK + ([({"F": 0}, -1), ({"F": 100}, -2), ({"F": 4160}, -2)] + each("w1 w2 packed", None, -1)
                                            + each("w1 w2 packed", P8, -2),),
    "rdetr_ffn_k256_pack_f32": FFN_PACK_F32 + (
        [({"F": 0}, -1), ({"rs1": 0}, -1), ({"cs2": 0}, -1), ({"F": 100}, -2), ({"b1": ONE}, -1), ({"b1": ONE, "b2": ONE}, -1), ({"packed": P8}, -2),
         ({"w1": P2}, -2), ({"w2": P2}, -2), ({"b1": P2, "b2": ONE, "biases": ONE}, -2), ({"b1": ONE, "b2": ONE, "biases": P17}, -2)]
        + each("w1 w2 packed", None, -1),),
    "rdetr_ffn_k256_bf16": FFN + (FFN_ROW_CASES,),
    "rdetr_ffn_ln_k256_bf16": FFN_LN + (
        FFN_ROW_CASES + each("gamma beta", None, -1)
        + [({"pos": ONE}, -1), ({"out2": ONE}, -1), ({"pos": ONE, "out2": ONE, "ldp": 255, "ldo2": 256}, -1),
           ({"pos": ONE, "out2": ONE, "ldp": 256, "ldo2": 255}, -1), ({"pos": ONE, "out2": ONE, "ldp": 260, "ldo2": 256}, -2),
           ({"pos": ONE, "out2": ONE, "ldp": 256, "ldo2": 260}, -2), ({"pos": P8, "out2": ONE, "ldp": 256, "ldo2": 256}, -2),
           ({"pos": ONE, "out2": P8, "ldp": 256, "ldo2": 256}, -2)],),
    "rdetr_ffn_k256_train_bf16": FFN_TRAIN + (
        FFN_ROW_CASES + [({"ldh": 2047}, -1), ({"ldh": 2052}, -2), ({"hid": None}, -1), ({"hid": P8}, -2), ({"M": 1 << 20}, -2)],),
    "rdetr_ffn_k256_train_xf32_bf16": FFN_TRAIN_XF32 + (
        [c for c in FFN_ROW_CASES if c[0] != {"ldx": 260}]         # fp32 rows: 260 floats IS a multiple of 16 bytes
        + [({"ldx": 258}, -2), ({"ldh": 2047}, -1), ({"ldh": 2052}, -2), ({"hid": None}, -1), ({"hid": P8}, -2), ({"ldxl": 255}, -1),
           ({"ldxl": 260}, -2), ({"xlp": None}, -1), ({"xlp": P8}, -2)],),
    "rdetr_ffn_k256_backward_bf16": FFN_BWD + (FFN_BWD_CASES + [({"lddx": 260}, -2)],),
    "rdetr_ffn_k256_backward_dxf32_bf16": FFN_BWD + (FFN_BWD_CASES + [({"lddx": 258}, -2)],),
    "rdetr_msda_forward_resident_bf16": RESIDENT + (
        [({"B": 0}, 0), ({"Nq": 0}, 0), ({"B": -1}, -1), ({"S": 0}, -1), ({"D": 64}, -2), ({"H": 4}, -2), ({"P": 8}, -2), ({"L": 3}, -2),
         ({"S": 9000, "Nq": 9000}, -2)] + each("value shapes starts loc attn out", None, -1) + each("value loc attn out", P8, -2),),
    "rdetr_msda_forward_fused_resident_bf16": RESIDENT_FUSED + (
        [({"B": 0}, 0), ({"Nq": 0}, 0), ({"B": -1}, -1), ({"ref_dim": 3}, -1), ({"ref_dim": 4}, -2), ({"ld_offs": 100}, -1), ({"ld_logits": 100}, -1),
         ({"ld_offs": 257}, -1), ({"ld_offs": 258}, -2), ({"ld_logits": 132}, -2), ({"D": 64}, -2)]
        + each("value shapes starts offs logits ref out", None, -1) + each("value offs logits ref out", P8, -2),),
}


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_refusal_before_any_hip_call(entry):
    names, base, cases = TABLE[entry]
    names = names.split()
    assert sorted(names) == sorted(base), entry                    # the row itself is well-formed
    fn = getattr(_lib.load(), entry)
    wrong = []
    for change, status in cases:
        assert set(change) <= set(names) | {"ldh"}, (entry, change)     # F past 4096 carries a hidden stride that fits it
        args = dict(base, **{k: v for k, v in change.items() if k in base})
        got = fn(*(args[n] for n in names))
        if got != status:
            wrong.append((change, got, status))
    assert not wrong, [(f"{c}: answered {g}, expected {s}") for c, g, s in wrong]
