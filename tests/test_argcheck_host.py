"""CPU tests of the argument checks of the entry points of attention.hip and elementwise.hip, built like test_gemm_argcheck_host.py:
one case per requirement an entry states, each refused with rc 1 and a message that starts with the name of the entry point that
was called and holds the text of that requirement, plus the empty problems with the return code each entry gives them - where an
entry checks before it looks at the size, an empty problem with a bad argument is refused, and where it looks at the size first
(rv_logp_finish_unpack, rv_next_token_scores) it is not.  The operands are made-up addresses: every case returns before anything
is launched (no GPU exists here, so a launch would be an error of its own, rc 2) - which is why calls that reach a launch whatever
their sizes (rv_grad_norm with n = 0, rv_clip_from_sumsq, rv_dpo_loss with B > 0, the resizes, rv_sum_rows_periodic) have no
passing or empty case here.  The three decode entry points have their cases in test_generate_host.py."""
import pytest

P = 0x7F0000010000          # an "operand": 64 KiB aligned, never dereferenced
ATTN = dict(qkv=P, ld=3072, q_col0=0, k_col0=1024, v_col0=2048, out=P, ldo=1024, lse=P, S=2, L=128, H=8, hd=128, scale=0.125,
            seg_sh=None, kv_group=1, row_off=None, row_len=None)
ATTN_BWD = dict(qkv=P, ld=3072, q_col0=0, k_col0=1024, v_col0=2048, dO=P, lddo=1024, O=P, ldo=1024, lse=P, delta=P, dqkv=P, lddq=3072,
                S=2, L=128, H=8, hd=128, causal=1, scale=0.125, seg_sh=None, seg_e1=None, kv_group=1, rope_cos=None, rope_sin=None,
                rope_pos=None, row_off=None, row_len=None)
RMS_BWD = dict(dy=P, lddy=64, x=P, ldx=64, row_idx=None, w=P, rstd=P, dres=None, lddres=0, dx=P, lddx=64, dw_partial=P, dw=P,
               dw_accumulate=0, rows=4, d=64)
NTS = dict(logits=P, ldl=1024, M=4, V_valid=1000, seen_off=None, seen_ids=None, penalty=1.0, want_ids=P, K=2, probs=P, logp=P,
           argmax=P, lse=P)
UNPACK = dict(pmax=P, psum=P, tgt_logit=P, nblk=4, M=8, dst_a=P, dst_b=P, dst_c=P, per_token=P, n_per_token=16, compact=P, n_compact=4)
SPAN = dict(L=1 << 20, ld=2048, q_col0=0, k_col0=0, v_col0=0)       # 2^20 rows of 4 KiB: 4.3e9 bytes

# name -> (a call that passes every check, [(what is wrong, overrides, the requirement's text)], [(empty problem, overrides, rc, text)])
ENTRIES = {
    "rv_set_attn_dkv_version": (
        dict(version=0),
        [("version 4", dict(version=4), "0 (environment / default), 3 or 5"), ("version 2", dict(version=2), "3 or 5"),
         ("version -1", dict(version=-1), "3 or 5")],
        [("version 0", dict(), 0, None)]),
    "rv_set_attn_fwd_version": (
        dict(version=0),
        [("version 5", dict(version=5), "0 (environment / default), 2 or 3"), ("version 1", dict(version=1), "2 or 3")],
        [("version 0", dict(), 0, None)]),
    "rv_attn_fwd": (
        dict(ATTN, causal=1, seg_e1=None),
        [("hd", dict(hd=96), "head dim must be 64 or 128"),
         ("row_off alone", dict(row_off=P), "row_off and row_len go together"),
         ("row_len alone", dict(row_len=P), "row_off and row_len go together"),
         ("kv_group 3", dict(kv_group=3), "kv_group must divide the number of query heads"),
         ("kv_group 0", dict(kv_group=0), "kv_group must divide the number of query heads"),
         ("ld", dict(ld=3076), "alignment"), ("ldo", dict(ldo=1028), "alignment"), ("q_col0", dict(q_col0=4), "alignment"),
         ("k_col0", dict(k_col0=1028), "alignment"), ("v_col0", dict(v_col0=2052), "alignment"),
         ("span", SPAN, "one sequence must span < 4 GB of the qkv buffer (32-bit DMA offsets)")],
        [("S = 0", dict(S=0), 0, None), ("L = 0", dict(L=0), 0, None), ("S = 0, bad hd", dict(S=0, hd=96), 1, "head dim must be 64 or 128"),
         ("L = 0, bad ld", dict(L=0, ld=3076), 1, "alignment")]),
    "rv_attn_fwd_branches": (
        dict(ATTN, seg_sh=P, q_lo=P),
        [("hd", dict(hd=96), "head dim must be 64 or 128"),
         ("seg_sh missing", dict(seg_sh=None), "seg_sh and q_lo are required"),
         ("q_lo missing", dict(q_lo=None), "seg_sh and q_lo are required"),
         ("row_off alone", dict(row_off=P), "row_off and row_len go together"),
         ("kv_group 3", dict(kv_group=3), "kv_group must divide the number of query heads"),
         ("ld", dict(ld=3076), "alignment"), ("ldo", dict(ldo=1028), "alignment"), ("k_col0", dict(k_col0=1028), "alignment"),
         ("span", SPAN, "one sequence must span < 4 GB of the qkv buffer (32-bit DMA offsets)")],
        [("S = 0", dict(S=0), 0, None), ("L = 0", dict(L=0), 0, None), ("S = 0, no q_lo", dict(S=0, q_lo=None), 1, "seg_sh and q_lo are required"),
         ("L = 0, bad kv_group", dict(L=0, kv_group=3), 1, "kv_group must divide the number of query heads")]),
    "rv_attn_bwd": (
        ATTN_BWD,
        [("hd", dict(hd=64), "head dim must be 128"),
         ("row_off alone", dict(row_off=P), "row_off and row_len go together"),
         ("pad-free rope without rope_pos", dict(row_off=P, row_len=P, rope_cos=P, rope_sin=P),
          "pad-free rows with the fused inverse rotation need the position table (rope_pos)"),
         ("rope_cos alone", dict(rope_cos=P), "rope_cos and rope_sin go together"),
         ("rope_sin alone", dict(rope_sin=P), "rope_cos and rope_sin go together"),
         ("O missing", dict(O=None), "O (forward output) and the delta workspace are required"),
         ("delta missing", dict(delta=None), "O (forward output) and the delta workspace are required"),
         ("ldo", dict(ldo=1028), "O (forward output) and the delta workspace are required"),
         ("kv_group 3", dict(kv_group=3), "kv_group must divide the number of query heads"),
         ("seg_sh alone", dict(seg_sh=P), "seg_sh and seg_e1 go together"),
         ("seg_e1 alone", dict(seg_e1=P), "seg_sh and seg_e1 go together"),
         ("ld", dict(ld=3076), "alignment"), ("lddo", dict(lddo=1028), "alignment"), ("lddq", dict(lddq=3076), "alignment"),
         ("span of qkv", dict(L=1 << 20, ld=2048, lddq=2048), "one sequence must span < 4 GB of the qkv / dO buffers"),
         ("span of dO", dict(L=1 << 20, ld=1024, lddo=2048), "one sequence must span < 4 GB of the qkv / dO buffers")],
        [("S = 0", dict(S=0), 0, None), ("L = 0", dict(L=0), 0, None), ("S = 0, bad hd", dict(S=0, hd=64), 1, "head dim must be 128"),
         ("L = 0, no O", dict(L=0, O=None), 1, "O (forward output) and the delta workspace are required")]),
    "rv_attn_delta": (
        dict(dO=P, lddo=1024, O=P, ldo=1024, delta=P, S=2, L=128, H=8, hd=128),
        [("hd", dict(hd=127), "hd even")],
        [("S = 0", dict(S=0), 0, None), ("L = 0", dict(L=0), 0, None), ("H = 0", dict(H=0), 0, None), ("S = 0, odd hd", dict(S=0, hd=127), 1, "hd even")]),
    "rv_rmsnorm_fwd": (
        dict(x=P, ldx=64, row_idx=None, w=P, y=P, ldy=64, rstd=P, rows=4, d=64, eps=1e-5),
        [("d", dict(d=60), "d/ld must be multiples of 8"), ("ldx", dict(ldx=68), "d/ld must be multiples of 8"),
         ("ldy", dict(ldy=68), "d/ld must be multiples of 8")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, bad d", dict(rows=0, d=60), 1, "d/ld must be multiples of 8")]),
    "rv_rmsnorm_fwd_dropout": (
        dict(x=P, ldx=64, row_idx=None, w=P, y=P, ldy=64, rstd=P, rows=4, d=64, eps=1e-5, yd=P, p=0.25, seed=3),
        [("d", dict(d=60), "d/ld must be multiples of 8"), ("ldy", dict(ldy=68), "d/ld must be multiples of 8"),
         ("yd missing", dict(yd=None), "yd required, 0 <= p < 1"), ("p = 1", dict(p=1.0), "yd required, 0 <= p < 1"),
         ("p < 0", dict(p=-0.5), "yd required, 0 <= p < 1")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, p = 1", dict(rows=0, p=1.0), 1, "yd required, 0 <= p < 1")]),
    "rv_rmsnorm_bwd": (
        RMS_BWD,
        [("d % 8", dict(d=60), "d must be a multiple of 8 and <= 8192"), ("d > 8192", dict(d=8200), "d must be a multiple of 8 and <= 8192"),
         ("lddy", dict(lddy=68), "ld alignment"), ("ldx", dict(ldx=68), "ld alignment"), ("lddx", dict(lddx=68), "ld alignment"),
         ("lddres", dict(lddres=68), "ld alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, bad ldx", dict(rows=0, ldx=68), 1, "ld alignment")]),
    "rv_rmsnorm_bwd_f32x": (
        RMS_BWD,
        [("d % 8", dict(d=60), "d must be a multiple of 8 and <= 8192"), ("d > 8192", dict(d=8200), "d must be a multiple of 8 and <= 8192"),
         ("lddy", dict(lddy=68), "ld alignment"), ("ldx", dict(ldx=66), "ld alignment"), ("lddx", dict(lddx=68), "ld alignment"),
         ("lddres", dict(lddres=68), "ld alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, ldx % 4 is enough", dict(rows=0, ldx=68), 0, None),
         ("rows = 0, bad ldx", dict(rows=0, ldx=66), 1, "ld alignment")]),
    "rv_rmsnorm_fwd_f32": (
        dict(x=P, ldx=64, row_idx=None, add=None, ldadd=0, xout=None, ldxout=0, w=P, y=P, ldy=64, rstd=P, rows=4, d=64, eps=1e-5),
        [("d % 8", dict(d=60), "d % 8, d <= 8192, ld alignment"), ("d > 8192", dict(d=8200), "d % 8, d <= 8192, ld alignment"),
         ("ldx", dict(ldx=66), "d % 8, d <= 8192, ld alignment"), ("ldy", dict(ldy=68), "d % 8, d <= 8192, ld alignment"),
         ("add without xout", dict(add=P, ldadd=64), "add needs xout (fp32) and aligned strides"),
         ("ldadd", dict(add=P, ldadd=68, xout=P, ldxout=64), "add needs xout (fp32) and aligned strides"),
         ("ldxout", dict(add=P, ldadd=64, xout=P, ldxout=66), "add needs xout (fp32) and aligned strides"),
         ("neither y nor add", dict(y=None), "nothing to write")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, nothing to write", dict(rows=0, y=None), 1, "nothing to write")]),
    "rv_add_f32_bf16": (
        dict(x=P, b=P, out=P, n=64),
        [("n", dict(n=60), "n%8")],
        [("n = 0", dict(n=0), 0, None)]),
    "rv_layernorm_fwd": (
        dict(x=P, ldx=64, w=P, b=P, y=P, ldy=64, rows=4, d=64, eps=1e-5),
        [("d", dict(d=60), "alignment"), ("ldx", dict(ldx=68), "alignment"), ("ldy", dict(ldy=68), "alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, bad ldx", dict(rows=0, ldx=68), 1, "alignment")]),
    "rv_layernorm_fwd_f32in": (
        dict(x=P, ldx=64, w=P, b=P, y=P, ldy=64, rows=4, d=64, eps=1e-5),
        [("d", dict(d=60), "alignment"), ("ldx", dict(ldx=66), "alignment"), ("ldy", dict(ldy=68), "alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, ldx % 4 is enough", dict(rows=0, ldx=68), 0, None),
         ("rows = 0, bad ldx", dict(rows=0, ldx=66), 1, "alignment")]),
    "rv_layernorm_bwd": (
        dict(dy=P, lddy=64, x=P, ldx=64, x_period=0, w=P, dx=P, lddx=64, partial=P, dw=P, db=P, accumulate=0, rows=4, d=64, eps=1e-5),
        [("d % 8", dict(d=60), "d must be a multiple of 8 and <= 8192"), ("d > 8192", dict(d=8200), "d must be a multiple of 8 and <= 8192"),
         ("lddy", dict(lddy=68), "ld alignment"), ("ldx", dict(ldx=68), "ld alignment"), ("lddx", dict(lddx=68), "ld alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, bad lddy", dict(rows=0, lddy=68), 1, "ld alignment")]),
    "rv_add_rows": (
        dict(x=P, ldx=64, p=P, ldp=64, period=4, y=P, ldy=64, rows=8, d=64),
        [("d", dict(d=60), "alignment / period"), ("ldx", dict(ldx=68), "alignment / period"), ("ldp", dict(ldp=68), "alignment / period"),
         ("ldy", dict(ldy=68), "alignment / period"), ("period", dict(period=0), "alignment / period")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, period = 0", dict(rows=0, period=0), 1, "alignment / period")]),
    "rv_sum_rows_periodic": (
        dict(x=P, ldx=64, period=4, reps=2, y=P, ldy=64, d=64),
        [("d", dict(d=60), "alignment"), ("ldx", dict(ldx=68), "alignment"), ("ldy", dict(ldy=68), "alignment"),
         ("period", dict(period=0), "alignment"), ("reps", dict(reps=0), "alignment")],
        []),
    "rv_rope_inplace": (
        dict(x=P, ld=1024, cos_tab=P, sin_tab=P, pos=None, n_tok=16, L=8, n_heads_total=8, hd=128, backward=0),
        [("hd", dict(hd=120), "hd%16, ld%8"), ("ld", dict(ld=1028), "hd%16, ld%8")],
        [("n_tok = 0", dict(n_tok=0), 0, None), ("n_heads_total = 0", dict(n_heads_total=0), 0, None),
         ("n_tok = 0, bad ld", dict(n_tok=0, ld=1028), 1, "hd%16, ld%8")]),
    "rv_swiglu_fwd": (
        dict(gu=P, ldgu=128, act=P, lda=64, rows=4, f=64, interleaved=0),
        [("f", dict(f=60), "alignment"), ("ldgu", dict(ldgu=132), "alignment"), ("lda", dict(lda=68), "alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, interleaved", dict(rows=0, interleaved=1), 0, None),
         ("rows = 0, bad f", dict(rows=0, f=60), 1, "alignment")]),
    "rv_swiglu_fwd_dropout": (
        dict(gu=P, ldgu=128, act=P, lda=64, rows=4, f=64, actd=P, p=0.25, seed=3),
        [("f", dict(f=60), "alignment"), ("lda", dict(lda=68), "alignment"), ("actd missing", dict(actd=None), "actd required, 0 <= p < 1"),
         ("p = 1", dict(p=1.0), "actd required, 0 <= p < 1"), ("p < 0", dict(p=-0.5), "actd required, 0 <= p < 1")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, no actd", dict(rows=0, actd=None), 1, "actd required, 0 <= p < 1")]),
    "rv_swiglu_bwd": (
        dict(dact=P, ldd=64, gu=P, ldgu=128, dgu=P, lddgu=128, rows=4, f=64, interleaved=0),
        [("f", dict(f=60), "alignment"), ("ldgu", dict(ldgu=132), "alignment"), ("ldd", dict(ldd=68), "alignment"),
         ("lddgu", dict(lddgu=132), "alignment")],
        [("rows = 0", dict(rows=0), 0, None), ("rows = 0, interleaved", dict(rows=0, interleaved=1), 0, None),
         ("rows = 0, bad ldd", dict(rows=0, ldd=68), 1, "alignment")]),
    "rv_gelu_fwd": (dict(x=P, y=P, n=64), [("n", dict(n=60), "n%8")], [("n = 0", dict(n=0), 0, None)]),
    "rv_gelu_bwd": (dict(dy=P, x=P, dx=P, n=64), [("n", dict(n=60), "n%8")], [("n = 0", dict(n=0), 0, None)]),
    "rv_dropout": (
        dict(x=P, y=P, acc=None, n=64, p=0.25, seed=3),
        [("n", dict(n=60), "n%8"), ("p = 1", dict(p=1.0), "0 <= p < 1"), ("p < 0", dict(p=-0.5), "0 <= p < 1"),
         ("neither y nor acc", dict(y=None), "need an output (y) or an accumulator (acc)")],
        [("n = 0", dict(n=0), 0, None), ("n = 0, p = 1", dict(n=0, p=1.0), 1, "0 <= p < 1"),
         ("n = 0, no output", dict(n=0, y=None), 1, "need an output (y) or an accumulator (acc)")]),
    "rv_resize_h_u8": (
        dict(src=P, H=32, W=32, y0=0, rows=8, bounds=P, kk=P, ksize=4, out_w=16, tmp=P),
        [("H", dict(H=0), "bad sizes"), ("W", dict(W=0), "bad sizes"), ("rows", dict(rows=0), "bad sizes"), ("y0", dict(y0=-1), "bad sizes"),
         ("y0 + rows > H", dict(y0=28), "bad sizes"), ("ksize", dict(ksize=0), "bad sizes"), ("out_w", dict(out_w=0), "bad sizes")],
        []),
    "rv_resize_v_norm_u8": (
        dict(tmp=P, rows=8, out_w=16, bounds=P, kk=P, ksize=4, out_h=16, table=P, out=P),
        [("rows", dict(rows=0), "bad sizes"), ("out_w", dict(out_w=0), "bad sizes"), ("out_h", dict(out_h=0), "bad sizes"),
         ("ksize", dict(ksize=0), "bad sizes")],
        []),
    "rv_transpose": (
        {"in": P, "ld_in": 64, "out": P, "ldo": 128, "R": 100, "C": 64},
        [("C", dict(C=60), "C, ld_in, ldo must be multiples of 8"), ("ld_in", dict(ld_in=68), "C, ld_in, ldo must be multiples of 8"),
         ("ldo % 8", dict(ldo=132), "C, ld_in, ldo must be multiples of 8"), ("ldo < roundup(R, 64)", dict(ldo=104), "ldo must be >= roundup(R,64)")],
        [("R = 0", dict(R=0), 0, None), ("C = 0", dict(C=0), 0, None), ("C = 0, small ldo", dict(C=0, ldo=104), 1, "ldo must be >= roundup(R,64)")]),
    "rv_splice_fwd": (
        dict(src=P, embed=P, feats=P, out=P, n_rows=8, d=64),
        [("d", dict(d=60), "d%8")],
        [("n_rows = 0", dict(n_rows=0), 0, None), ("n_rows = 0, bad d", dict(n_rows=0, d=60), 1, "d%8")]),
    "rv_embed_bwd": (
        dict(uniq_ids=P, seg_off=P, pos_sorted=P, n_uniq=8, dx=P, dW=P, d=64),
        [("d", dict(d=60), "d%8")],
        [("n_uniq = 0", dict(n_uniq=0), 0, None), ("n_uniq = 0, bad d", dict(n_uniq=0, d=60), 1, "d%8")]),
    "rv_feat_grad": (
        dict(src_a=P, src_b=P, dx=P, dfeat=P, n_rows=8, d=64),
        [("d", dict(d=60), "d%8")],
        [("n_rows = 0", dict(n_rows=0), 0, None), ("n_rows = 0, bad d", dict(n_rows=0, d=60), 1, "d%8")]),
    "rv_gather_rows": (
        {"in": P, "ld_in": 64, "idx": P, "out": P, "ld_out": 64, "n_rows": 8, "d": 64, "scatter": 0},
        [("d", dict(d=60), "alignment"), ("ld_in", dict(ld_in=68), "alignment"), ("ld_out", dict(ld_out=68), "alignment")],
        [("n_rows = 0", dict(n_rows=0), 0, None), ("n_rows = 0, bad ld_out", dict(n_rows=0, ld_out=68), 1, "alignment")]),
    "rv_colsum": (dict(dy=P, ld=64, db=P, M=8, N=64), [], [("N = 0", dict(N=0), 0, None)]),
    "rv_im2col_patches": (
        dict(pixels=P, out=P, B=2, image_size=28, patch=14, Kp=640),
        [("image_size % patch", dict(image_size=30), "bad geometry"), ("Kp", dict(Kp=576), "bad geometry")],
        [("B = 0", dict(B=0), 0, None), ("B = 0, small Kp", dict(B=0, Kp=576), 1, "bad geometry")]),
    "rv_clip_assemble": (
        dict(patch=P, cls=P, pos=P, x=P, B=2, P=4, d=64),
        [("d", dict(d=60), "d%8")],
        [("B = 0", dict(B=0), 0, None), ("B = 0, bad d", dict(B=0, d=60), 1, "d%8")]),
    "rv_grad_norm": (dict(g=P, n=64, partial=P, max_norm=1.0, pre_scale=1.0, out2=P), [("n", dict(n=60), "n%8")], []),
    "rv_grad_sumsq": (dict(g=P, n=64, partial=P, out1=P, accumulate=0), [("n", dict(n=60), "n%8")], []),
    "rv_grad_accum": (
        dict(acc=P, g=P, n=64, mode=0, scale=1.0),
        [("n", dict(n=60), "n % 8 == 0, mode in 0..2"), ("mode 3", dict(mode=3), "n % 8 == 0, mode in 0..2"),
         ("mode -1", dict(mode=-1), "n % 8 == 0, mode in 0..2")],
        [("n = 0", dict(n=0), 0, None), ("n = 0, bad mode", dict(n=0, mode=3), 1, "n % 8 == 0, mode in 0..2")]),
    "rv_adamw_step": (
        dict(p=P, master=P, m=P, v=P, g=P, n=64, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, clip=None),
        [("n", dict(n=60), "n%8")],
        [("n = 0", dict(n=0), 0, None)]),
    "rv_logp_finish": (dict(pmax=P, psum=P, tgt_logit=P, nblk=4, M=8, lse=P, logp=P), [], [("M = 0", dict(M=0), 0, None)]),
    "rv_logp_finish_unpack": (
        UNPACK,
        [("nblk", dict(nblk=0), "nblk, M > 0; sizes >= 0"), ("M < 0", dict(M=-1), "nblk, M > 0; sizes >= 0"),
         ("n_per_token", dict(n_per_token=-1), "nblk, M > 0; sizes >= 0"), ("n_compact", dict(n_compact=-1), "nblk, M > 0; sizes >= 0"),
         ("dst_a missing", dict(dst_a=None), "the three destination tables are required (-1 = no slot)"),
         ("dst_c missing", dict(dst_c=None), "the three destination tables are required (-1 = no slot)"),
         ("per_token missing", dict(per_token=None), "NULL output with a non-zero size"),
         ("compact missing", dict(compact=None), "NULL output with a non-zero size")],
        [("M = 0", dict(M=0), 0, None), ("M = 0 goes before the checks: bad nblk", dict(M=0, nblk=0), 0, None),
         ("M = 0 goes before the checks: no tables", dict(M=0, dst_a=None, dst_b=None, dst_c=None), 0, None)]),
    "rv_next_token_scores": (
        NTS,
        [("M < 0", dict(M=-1), "M, V_valid > 0, ldl >= V_valid, K >= 0"), ("V_valid", dict(V_valid=0), "M, V_valid > 0, ldl >= V_valid, K >= 0"),
         ("ldl", dict(ldl=512), "M, V_valid > 0, ldl >= V_valid, K >= 0"), ("K", dict(K=-1), "M, V_valid > 0, ldl >= V_valid, K >= 0"),
         ("logits missing", dict(logits=None), "NULL buffer"), ("argmax missing", dict(argmax=None), "NULL buffer"),
         ("lse missing", dict(lse=None), "NULL buffer"), ("want_ids missing", dict(want_ids=None), "NULL buffer"),
         ("probs missing", dict(probs=None), "NULL buffer"),
         ("penalty", dict(penalty=0.0), "the repetition penalty must be positive (1 = off)"),
         ("seen_off alone", dict(seen_off=P), "seen_off without seen_ids"),
         ("bitmap", dict(seen_off=P, seen_ids=P, penalty=1.2, V_valid=480032, ldl=480032), "the seen-id bitmap (V_valid / 8 bytes) must fit in LDS")],
        [("M = 0", dict(M=0), 0, None), ("M = 0 goes before the checks: bad penalty", dict(M=0, penalty=0.0), 0, None),
         ("M = 0 goes before the checks: no buffers", dict(M=0, logits=None, argmax=None, lse=None), 0, None)]),
    "rv_seq_sum": (dict(logp=P, weight=None, seq_off=P, n_seq=4, out_sum=P, out_cnt=P), [], [("n_seq = 0", dict(n_seq=0), 0, None)]),
    "rv_dpo_loss": (
        dict(seq_sum=P, seq_cnt=P, ref_win=P, ref_rej=P, B=2, beta=0.1, use_average=0, sft_weight=0.0, dpo_weight=1.0, per_pair=P, scalars=P, coef=P),
        [("B = 0", dict(B=0), "B must be > 0"), ("B < 0", dict(B=-1), "B must be > 0")],
        []),
    "rv_row_coef": (dict(coef=P, seq_of_row=P, weight=None, out=P, n=8), [], [("n = 0", dict(n=0), 0, None)]),
    "rv_cast_f32_to_bf16": ({"in": P, "out": P, "n": 8}, [], [("n = 0", dict(n=0), 0, None)]),
    "rv_cast_bf16_to_f32": ({"in": P, "out": P, "n": 8}, [], [("n = 0", dict(n=0), 0, None)]),
    "rv_reduce_copy_persistent": (
        dict(a=P, b=P, dst=P, n=64, n_wg=4),
        [("n", dict(n=60), "n must be a multiple of 8 bf16 elements"), ("n_wg = 0", dict(n_wg=0), "1 <= n_wg <= 256"),
         ("n_wg = 257", dict(n_wg=257), "1 <= n_wg <= 256")],
        [("n = 0", dict(n=0), 0, None), ("n = 0, bad n_wg", dict(n=0, n_wg=0), 1, "1 <= n_wg <= 256")]),
}

# entry points of the two files that take no stream or check nothing and have no empty problem
NO_CASES = {"rv_attn_bwd_workspace_floats", "rv_rmsnorm_bwd_nblocks", "rv_sumsq_nblocks", "rv_clip_from_sumsq"}

REJECTED = [(name, what, over, text) for name, (_, bad, _) in ENTRIES.items() for what, over, text in bad]
EMPTY = [(name, what, over, rc, text) for name, (_, _, empty) in ENTRIES.items() for what, over, rc, text in empty]


def _lib():
    import __graft_entry__ as g
    g.build()
    from rlaif_v_amd import hip
    return hip.lib()


def call(lib, name, over):
    """(rc, message) of the entry point on its passing call with ``over`` applied; the stream is NULL"""
    kw = dict(ENTRIES[name][0], **over)
    names = [a for _, a in lib.decls[name][1]]
    assert set(kw) | ({"stream"} & set(names)) == set(names), (name, sorted(set(names) ^ set(kw)))
    rc = getattr(lib.lib, name)(*[kw.get(a) for a in names])
    return rc, lib.last_error()


def _entry_points_of(*sources):
    """the rv_* functions the given translation units define"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rlaif-v_amd", "csrc")
    text = "".join(open(os.path.join(csrc, s)).read() for s in sources)
    return set(re.findall(r"^(?:extern \"C\" )?(?:int|long) (rv_\w+)\(", text, flags=re.M))


def test_the_table_covers_every_entry_point_of_the_two_files():
    lib = _lib()
    want = _entry_points_of("attention.hip", "elementwise.hip")
    assert want <= set(lib.decls) and len(want) > 40
    assert want - NO_CASES == set(ENTRIES)


def test_the_table_has_a_case_for_every_requirement_of_the_two_files():
    """every message of an RV_REQUIRE line, and of the checks rv_attn_fwd and rv_attn_fwd_branches share, is some case's text"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rlaif-v_amd", "csrc")
    texts = {(n, t) for n, _, _, t in REJECTED}
    for src in ("attention.hip", "elementwise.hip"):
        code = open(os.path.join(csrc, src)).read()
        for msg in re.findall(r"\"(rv_\w+: [^\"]+)\"\);", code):
            name, text = msg.split(": ", 1)
            assert (name, text) in texts, msg


@pytest.mark.parametrize("name,what,over,text", REJECTED, ids=[f"{n}-{w}" for n, w, _, _ in REJECTED])
def test_bad_arguments_are_refused_by_name_without_a_launch(name, what, over, text):
    rc, msg = call(_lib(), name, over)
    assert rc == 1, (name, what, rc, msg)
    assert msg.startswith(name + ": "), (name, what, msg)
    assert text in msg[len(name) + 2:], (name, what, msg)


@pytest.mark.parametrize("name,what,over,want,text", EMPTY, ids=[f"{n}-{w}" for n, w, _, _, _ in EMPTY])
def test_empty_problems(name, what, over, want, text):
    rc, msg = call(_lib(), name, over)
    assert rc == want, (name, what, rc, msg)
    if want:
        assert msg.startswith(name + ": "), (name, what, msg)
        assert text in msg[len(name) + 2:], (name, what, msg)
