"""CPU tests of the argument checks of every GEMM entry point of gemm.hip (``rv_gemm_*`` and the two ``rv_lmhead_logp_*``): one
case per requirement an entry states, each refused with rc 1 and a message that names the entry point that was called, plus the
empty problems with the return code each entry gives them.  The operands are made-up addresses: every case returns before
anything is launched (no GPU exists here, so a launch would be an error of its own, rc 2).  rv_gemm_nt_skinny_bf16 lives with the
decode kernels and has its cases in test_generate_host.py; rv_gemm_tn_workspace_floats checks nothing."""
import re

import pytest

P = 0x7F0000010000          # an "operand": 64 KiB aligned, never dereferenced
NT = dict(A=P, lda=128, B=P, ldb=128, M=128, N=128, K=128)
NN = dict(A=P, lda=512, B=P, ldb=512, M=128, N=512, K=512)
EXT = dict(A2=P, lda2=64, B2=P, K2=64)
TN = dict(P=P, ldp=128, Q=P, ldq=128, C=P, ldc=128, R=256, I=128, J=128)

# name -> (a call that passes every check, [(what is wrong, overrides)], [(empty problem, overrides, rc)])
# "what is wrong" begins with the argument at fault, and says what the message has to say: see said_why()
ENTRIES = {
    "rv_gemm_nt_bf16": (
        dict(NT, C=P, ldc=128, bias=None, residual=None, ldr=0, act=0, alpha=1.0, variant=-1),
        [("K", dict(K=96)), ("K = 0", dict(K=0)), ("N", dict(N=130)), ("lda", dict(lda=132)), ("ldc", dict(ldc=130)),
         ("ldr", dict(residual=P, ldr=130)), ("A", dict(A=P + 8)), ("B", dict(B=P + 8)), ("variant", dict(variant=4))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0), ("M = 0, bad K", dict(M=0, K=96), 0)]),
    "rv_gemm_nt_bf16_f32out": (
        dict(NT, C=P, ldc=128, variant=-1),
        [("K", dict(K=96)), ("N", dict(N=130)), ("ldb", dict(ldb=132)), ("ldc", dict(ldc=130)), ("A", dict(A=P + 8)),
         ("variant", dict(variant=4))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nt_bf16_f32res": (
        dict(NT, C=P, ldc=128, bias=None, residual=P, ldr=128, variant=-1),
        [("K", dict(K=96)), ("N", dict(N=130)), ("lda", dict(lda=132)), ("ldc", dict(ldc=130)), ("ldr", dict(ldr=130)),
         ("B", dict(B=P + 8)), ("variant", dict(variant=4))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nt_dropout_bf16": (
        dict(NT, C=P, ldc=128, residual=None, ldr=0, alpha=1.0, p=0.25, seed=3),
        [("K", dict(K=96)), ("N % 4", dict(N=130)), ("N % 8", dict(N=132)), ("lda", dict(lda=132)), ("ldc", dict(ldc=130)),
         ("ldr", dict(residual=P, ldr=130)), ("B", dict(B=P + 8)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0), ("M = 0, bad p", dict(M=0, p=1.0), 0)]),
    "rv_gemm_nt_lora_bf16": (
        dict(NT, **EXT, ldb2=64, group_cols=0, group0=0, C=P, ldc=128, N=384, residual=None, ldr=0),
        [("K", dict(K=96)), ("N", dict(N=130)), ("K2", dict(K2=32)), ("K2 = 0", dict(K2=0)), ("lda", dict(lda=132)),
         ("lda2", dict(lda2=68)), ("ldb2", dict(ldb2=68)), ("ldc", dict(ldc=130)), ("ldr", dict(residual=P, ldr=130)),
         ("A2", dict(A2=P + 8)), ("B2", dict(B2=P + 8)), ("group_cols % 128", dict(group_cols=64)),
         ("group_cols does not tile N", dict(group_cols=256)), ("group0 % 128", dict(group_cols=128, group0=64)),
         ("group0 > N", dict(group_cols=128, group0=512))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_bf16": (
        dict(NN, C=P, ldc=512, residual=None, ldr=0, alpha=1.0),
        [("K", dict(K=48)), ("K = 0", dict(K=0)), ("N", dict(N=12)), ("lda", dict(lda=516)), ("ldb", dict(ldb=516)),
         ("ldc", dict(ldc=514)), ("ldr", dict(residual=P, ldr=514)), ("A", dict(A=P + 8)), ("B", dict(B=P + 8))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_bias_act_bf16": (
        dict(NN, C=P, ldc=512, bias=P, residual=None, ldr=0, act=1, alpha=1.0),
        [("K", dict(K=48)), ("N", dict(N=12)), ("lda", dict(lda=516)), ("ldc", dict(ldc=514)), ("ldr", dict(residual=P, ldr=514)),
         ("A", dict(A=P + 8)), ("bias", dict(bias=P + 8)), ("activation", dict(act=7))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0), ("M = 0, bad activation", dict(M=0, act=7), 1),
         ("N = 0, bad bias", dict(N=0, bias=P + 8), 1)]),
    "rv_gemm_nn_rope_bf16": (
        dict(NN, C=P, ldc=512, cos_tab=P, sin_tab=P, pos=None, L=64, rope_cols=256, hd=128),
        [("hd", dict(hd=64)), ("K < 512", dict(K=256)), ("K % 64", dict(K=544)), ("N", dict(N=384)), ("rope_cols", dict(rope_cols=128)),
         ("rope_cols > N", dict(rope_cols=768)), ("lda", dict(lda=516)), ("ldc", dict(ldc=516)), ("C", dict(C=P + 8)),
         ("cos_tab", dict(cos_tab=P + 8)), ("cos_tab missing", dict(cos_tab=None)), ("L", dict(L=0))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_swiglu_bf16": (
        dict(NN, GU=P, ldgu=512, ACT=P, ldact=256),
        [("K", dict(K=48)), ("N", dict(N=24)), ("lda", dict(lda=516)), ("ldgu", dict(ldgu=516)), ("ldact", dict(ldact=258)),
         ("A", dict(A=P + 8)), ("GU", dict(GU=P + 8)), ("ACT", dict(ACT=P + 4))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_swiglu_bwd_bf16": (
        dict(NN, GU=P, ldgu=1024, DGU=P, lddgu=1024),
        [("K", dict(K=48)), ("N", dict(N=12)), ("ldb", dict(ldb=516)), ("ldgu", dict(ldgu=1028)), ("lddgu", dict(lddgu=1028)),
         ("B", dict(B=P + 8)), ("GU", dict(GU=P + 8)), ("DGU", dict(DGU=P + 8))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_lora_bf16": (
        dict(NN, **EXT, ldb2=512, group_cols=0, group0=0, C=P, ldc=512, residual=None, ldr=0),
        [("K", dict(K=48)), ("K2", dict(K2=48)), ("K2 = 0", dict(K2=0)), ("N", dict(N=12)), ("lda", dict(lda=516)),
         ("lda2", dict(lda2=68)), ("ldb2", dict(ldb2=516)), ("ldc", dict(ldc=514)), ("ldr", dict(residual=P, ldr=514)),
         ("A", dict(A=P + 8)), ("A2", dict(A2=P + 8)), ("B2", dict(B2=P + 8)), ("group_cols % 256", dict(group_cols=128)),
         ("group_cols does not tile N", dict(N=768, group_cols=512)), ("group0 % 256", dict(group_cols=256, group0=128))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_lora_swiglu_bf16": (
        dict(NN, **EXT, ldb2=512, GU=P, ldgu=512, ACT=P, ldact=256, ACTD=None, p=0.25, seed=3),
        [("K < 512", dict(K=256)), ("K % 64", dict(K=544)), ("K2", dict(K2=32)), ("N", dict(N=24)), ("lda", dict(lda=516)),
         ("lda2", dict(lda2=68)), ("ldgu", dict(ldgu=516)), ("ldact", dict(ldact=258)), ("A2", dict(A2=P + 8)), ("GU", dict(GU=P + 8)),
         ("ACT", dict(ACT=P + 4)), ("ACTD", dict(ACTD=P + 4)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5)),
         ("ACTD with a strided ACT", dict(ACTD=P, ldact=264))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_lora_swiglu_bwd_bf16": (
        dict(NN, **EXT, ldb2=512, p=0.25, seed=3, GU=P, ldgu=1024, DGU=P, lddgu=1024),
        [("K < 512", dict(K=256)), ("K2", dict(K2=32)), ("N", dict(N=12)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5)),
         ("ldb2", dict(ldb2=516)), ("lddgu", dict(lddgu=1028)), ("B2", dict(B2=P + 8)), ("DGU", dict(DGU=P + 8))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_nn_lora_pre_bf16": (
        dict(NN, **EXT, ldb2=512, group_cols=0, group0=0, p=0.25, seed=3, C=P, ldc=512, residual=None, ldr=0),
        [("K < 512", dict(K=256)), ("K % 64", dict(K=544)), ("K2", dict(K2=32)), ("N", dict(N=12)), ("p = 1", dict(p=1.0)),
         ("p < 0", dict(p=-0.5)), ("lda2", dict(lda2=68)), ("ldc", dict(ldc=514)), ("ldr", dict(residual=P, ldr=514)),
         ("A2", dict(A2=P + 8)), ("group_cols % 256", dict(group_cols=128)), ("group0 % 256", dict(group_cols=256, group0=128))],
        [("M = 0", dict(M=0), 0), ("N = 0", dict(N=0), 0)]),
    "rv_gemm_tn_bf16": (
        dict(TN, residual=None, ldr=0, alpha=1.0),
        [("R", dict(R=0)), ("I", dict(I=12)), ("J", dict(J=4)), ("ldp", dict(ldp=132)), ("ldc", dict(ldc=130)),
         ("ldr", dict(residual=P, ldr=130)), ("P", dict(P=P + 8)), ("Q", dict(Q=P + 8))],
        [("I = 0", dict(I=0), 0), ("J = 0", dict(J=0), 0), ("I = 0, R = 0", dict(I=0, R=0), 0)]),
    "rv_gemm_tn_bf16_ws": (
        dict(TN, workspace=P, workspace_floats=1 << 20),
        [("R", dict(R=0)), ("I", dict(I=12)), ("ldq", dict(ldq=132)), ("ldc", dict(ldc=130)), ("Q", dict(Q=P + 8)),
         ("workspace", dict(workspace=P + 8)), ("C", dict(C=P + 4))],
        [("I = 0", dict(I=0), 0), ("J = 0", dict(J=0), 0)]),
    "rv_gemm_tn_bf16_splitk": (
        dict(TN, alpha=1.0, splits=4, workspace=P),
        [("R", dict(R=0)), ("splits = 0", dict(splits=0)), ("splits > 1024", dict(splits=1025)), ("I", dict(I=12)), ("J", dict(J=12)),
         ("ldp", dict(ldp=132)), ("ldc", dict(ldc=130)), ("P", dict(P=P + 8)), ("workspace", dict(workspace=P + 8)),
         ("workspace missing", dict(workspace=None))],
        [("I = 0", dict(I=0), 0), ("J = 0", dict(J=0), 0)]),
    "rv_gemm_nt_lora_masks_bf16": (
        dict(X=P, ldx=256, A=P, lda=256, T=P, ldt=128, M=128, K=256, G=2, alpha=1.0, p=0.25, seed0=1, seed1=2, seed2=3),
        [("G = 0", dict(G=0)), ("G = 4", dict(G=4)), ("K", dict(K=96)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5)),
         ("ldx % 8", dict(ldx=260)), ("ldx < K", dict(ldx=128)), ("ldt % 4", dict(ldt=130)), ("ldt < 64 G", dict(ldt=64)),
         ("M < 0", dict(M=-1)), ("X missing", dict(X=None)), ("X", dict(X=P + 8)), ("T", dict(T=P + 4))],
        [("M = 0", dict(M=0), 0), ("M = 0, no operands", dict(M=0, X=None, A=None, T=None), 0), ("M = 0, bad G", dict(M=0, G=4), 1),
         ("M = 0, bad p", dict(M=0, p=1.0), 1)]),
    "rv_gemm_nt_dropout_masks_bf16": (
        dict(dT=P, lddt=128, AT=P, ldat=128, C=P, ldc=256, M=128, N=256, G=2, residual=None, ldr=0, p=0.25, seed0=1, seed1=2, seed2=3),
        [("G = 0", dict(G=0)), ("G = 4", dict(G=4)), ("N", dict(N=96)), ("N = 0", dict(N=0)), ("p = 1", dict(p=1.0)),
         ("p < 0", dict(p=-0.5)), ("lddt % 8", dict(lddt=132)), ("ldat < 64 G", dict(ldat=64)), ("ldc < N", dict(ldc=128)),
         ("ldr % 4", dict(residual=P, ldr=258)), ("dT missing", dict(dT=None)), ("AT", dict(AT=P + 8)), ("C", dict(C=P + 4)),
         ("residual", dict(residual=P + 4, ldr=256))],
        [("M = 0", dict(M=0), 0), ("M = 0, bad p", dict(M=0, p=1.0), 1), ("M = 0, bad N", dict(M=0, N=96), 1)]),
    "rv_gemm_tn_lora_masks_bf16": (
        dict(dT=P, lddt=128, X=P, ldx=256, dA=P, ldda=256, R=512, K=256, G=2, p=0.25, seed0=1, seed1=2, seed2=3, splits=4, workspace=P),
        [("G = 0", dict(G=0)), ("G = 4", dict(G=4)), ("K", dict(K=96)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5)),
         ("R", dict(R=0)), ("splits = 0", dict(splits=0)), ("splits > 1024", dict(splits=1025)), ("lddt < 64 G", dict(lddt=64)),
         ("ldx % 8", dict(ldx=260)), ("ldda % 4", dict(ldda=258)), ("X missing", dict(X=None)), ("dT", dict(dT=P + 8)),
         ("dA", dict(dA=P + 4)), ("workspace", dict(workspace=P + 8)), ("workspace missing", dict(workspace=None)),
         ("workspace missing, p = 0", dict(workspace=None, p=0.0))],
        []),
    "rv_lmhead_logp_fwd": (
        dict(h=P, ldh=128, W=P, ldw=128, tgt=P, M=128, V=256, V_valid=250, K=128, pmax=P, psum=P, tgt_logit=P, variant=-1),
        [("K", dict(K=96)), ("N % 4 (N is V)", dict(V=130, V_valid=130)), ("V % 64", dict(V=96, V_valid=96)), ("V_valid <= V - 64", dict(V_valid=192)),
         ("V_valid > V", dict(V_valid=257)), ("ldh", dict(ldh=132)), ("W", dict(W=P + 8)), ("variant", dict(variant=4))],
        [("M = 0", dict(M=0), 0), ("M = 0, bad K", dict(M=0, K=96), 0)]),
    "rv_lmhead_logp_bwd": (
        dict(h=P, ldh=128, W=P, ldw=128, tgt=P, lse=P, coef=P, dlogits=P, ldd=256, M=128, V=256, V_valid=250, K=128, variant=-1),
        [("K", dict(K=96)), ("N % 4 (N is V)", dict(V=130, V_valid=130)), ("ldd", dict(ldd=258)), ("V_valid <= V - 64", dict(V_valid=192)),
         ("V_valid > V", dict(V_valid=257)), ("ldw", dict(ldw=132)), ("h", dict(h=P + 8)), ("variant", dict(variant=4))],
        [("M = 0", dict(M=0), 0)]),
}

REJECTED = [(name, what, over) for name, (_, bad, _) in ENTRIES.items() for what, over in bad]
EMPTY = [(name, what, over, rc) for name, (_, _, empty) in ENTRIES.items() for what, over, rc in empty]


def _lib():
    import __graft_entry__ as g
    g.build()
    from rlaif_v_amd import hip
    return hip.lib()


def call(lib, name, over):
    """(rc, message) of the entry point on its passing call with ``over`` applied; the stream is NULL"""
    kw = dict(ENTRIES[name][0], **over)
    names = [a for _, a in lib.decls[name][1]]
    assert set(kw) | {"stream"} == set(names), (name, sorted(set(names) ^ set(kw)))
    rc = getattr(lib.lib, name)(*[kw.get(a) for a in names])
    return rc, lib.last_error()


def said_why(what, over, msg):
    """Did ``msg`` (the entry point's name taken off) give the requirement that the case ``what`` breaks?  A misaligned leading
    dimension must read "leading dimension", a misaligned address "-byte aligned", and every other case must name, as a word of
    its own, the argument its label begins with - so a case that is refused for another reason than its label says fails."""
    arg = what.split()[0].rstrip(",")
    if arg.startswith("ld"):
        return "leading dimension" in msg
    if isinstance(over.get(arg), int) and over[arg] > P and over[arg] % 16:          # P + 4, P + 8
        return "-byte aligned" in msg
    return re.search(rf"(?<![A-Za-z0-9_]){re.escape(arg)}(?![A-Za-z0-9_])", msg) is not None


def test_the_table_covers_every_gemm_entry_point_of_the_header():
    lib = _lib()
    want = {n for n in lib.decls if n.startswith(("rv_gemm_", "rv_lmhead_logp_"))} - {"rv_gemm_tn_workspace_floats", "rv_gemm_nt_skinny_bf16"}
    assert want == set(ENTRIES)


@pytest.mark.parametrize("name,what,over", REJECTED, ids=[f"{n}-{w}" for n, w, _ in REJECTED])
def test_bad_arguments_are_refused_by_name_without_a_launch(name, what, over):
    rc, msg = call(_lib(), name, over)
    assert rc == 1, (name, what, rc, msg)
    assert msg.startswith(name + ":"), (name, what, msg)
    assert said_why(what, over, msg[len(name) + 1:]), (name, what, msg)


@pytest.mark.parametrize("name,what,over,want", EMPTY, ids=[f"{n}-{w}" for n, w, _, _ in EMPTY])
def test_empty_problems(name, what, over, want):
    rc, msg = call(_lib(), name, over)
    assert rc == want, (name, what, rc, msg)
    if want:
        assert msg.startswith(name + ":"), (name, what, msg)
        assert said_why(what.split(", ")[-1].replace("bad ", ""), over, msg[len(name) + 1:]), (name, what, msg)
