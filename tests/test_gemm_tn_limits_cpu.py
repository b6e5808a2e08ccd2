"""CPU: the argument validation of made_gemm_tn_grouped's workspace form (rejected before any HIP call, fake non-null pointers).

The first launch of the 256 x 256-tile workspace form addresses its partial slots with 32-bit byte offsets (csrc/gemm_tn_glds.hip flush_ws),
so a group whose workspace reaches 2^32 bytes must be refused: eight problems with N = K = 4096 at M = 36864 are 2048 tiles on a grid of
256 workgroups, 65 slots of 256 KB each = 4.36e9 bytes."""
import ctypes as C
import os

from mgsv_amd import _lib

FAKE = 4096          # a non-null, 16-byte aligned "device pointer": validation rejects the call before anything reads it
INVALID, UNSUPPORTED = -1, -2


def _lib_built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _group(n_problems, N=4096, K=4096, M=36864):
    g = _lib.MadeGemmTNGroup()
    g.n_problems, g.alpha, g.M, g.split_m, g.tile_size = n_problems, 1.0, M, 1, 256
    for i in range(n_problems):
        p = g.p[i]
        p.A, p.B, p.C = FAKE, FAKE, FAKE
        p.N, p.K, p.lda, p.ldb, p.ldc = N, K, N, K, K
    return g


def test_grouped_workspace_of_4_gib_or_more_is_refused():
    l = _lib_built()
    g = _group(8)
    need = int(l.made_gemm_tn_grouped_workspace(C.byref(g)))
    assert need == 256 * 65 * 262144 and need >= 2 ** 32
    g.workspace, g.workspace_bytes = FAKE, need
    assert l.made_gemm_tn_grouped(C.byref(g), None) == UNSUPPORTED
    msg = l.made_last_error().decode()
    assert "2^32" in msg and str(need) in msg, msg


def test_grouped_workspace_of_half_that_size_passes_the_limit():
    """Four such problems need 2.2e9 bytes (past 2^31, below 2^32: the offsets are unsigned).  The call is then turned down for the next
    thing validation looks at -- a workspace one byte short -- which shows that the limit let it through, still before any HIP call."""
    l = _lib_built()
    g = _group(4)
    need = int(l.made_gemm_tn_grouped_workspace(C.byref(g)))
    assert need == 256 * 33 * 262144 and 2 ** 31 < need < 2 ** 32
    g.workspace, g.workspace_bytes = FAKE, need - 1
    assert l.made_gemm_tn_grouped(C.byref(g), None) == INVALID
    msg = l.made_last_error().decode()
    assert "2^32" not in msg and f"{need} needed" in msg, msg

