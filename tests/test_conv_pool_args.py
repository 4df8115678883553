"""CPU: conv3x3_fwd, conv3x3_wgrad, conv3x3_pool_fwd and the pooled BatchNorm entries reject bad arguments before any launch (no GPU is touched: the
pointers are made-up, 16-byte aligned addresses that a launch would fault on)."""
from src import _native as N

A = 4096          # a non-null, aligned address


def pool_fwd(X=A, W=A, bias=A, gamma=A, Y=A, Praw=A, s=A, q=A + 512, rep=8, n=3, Ti=6, Fi=32):
    return N.lib().audiossl_conv3x3_pool_fwd(X, W, bias, gamma, Y, Praw, s, q, rep, n, Ti, Fi, None)


def test_conv_pool_fwd_rejects_what_it_cannot_pool():
    assert pool_fwd(Ti=5) == -1 and pool_fwd(Ti=25) == -1           # a window would straddle two waves' rows
    assert pool_fwd(Fi=8) == -1 and pool_fwd(Fi=64) == -1
    assert pool_fwd(Praw=None) == -1
    assert pool_fwd(gamma=None) == -1 and pool_fwd(s=None, q=None) == -1 and pool_fwd(q=None) == -1
    assert pool_fwd(X=None) == -1 and pool_fwd(W=None) == -1 and pool_fwd(n=0) == -1 and pool_fwd(Ti=0) == -1
    assert pool_fwd(q=A + 1024) == -1 and pool_fwd(rep=0) == -1 and pool_fwd(rep=65) == -1      # replicas: sumsq == sum + 64 doubles
    assert pool_fwd(n=1 << 20, Ti=64) == -1                         # past the 2 GB a 32-bit buffer offset reaches
    assert pool_fwd(Praw=A + 8) == -3 and pool_fwd(Y=A + 2) == -3


def conv_fwd(X=A, W=A, bias=A, Y=A, f32=0, s=A, q=A + 512, rep=1, n=3, Ti=6, Fi=32):
    return N.lib().audiossl_conv3x3_fwd(X, W, bias, Y, f32, s, q, rep, n, Ti, Fi, None)


def test_conv_fwd_rejects_bad_arguments():
    assert conv_fwd(X=None) == -1 and conv_fwd(W=None) == -1 and conv_fwd(Y=None) == -1
    assert conv_fwd(n=0) == -1 and conv_fwd(n=-1) == -1 and conv_fwd(Ti=0) == -1 and conv_fwd(Ti=-3) == -1
    assert conv_fwd(Fi=8) == -1 and conv_fwd(Fi=64) == -1 and conv_fwd(Fi=0) == -1 and conv_fwd(Fi=24) == -1
    assert conv_fwd(q=None) == -1 and conv_fwd(s=None) == -1                # the statistics come as a pair or not at all
    assert conv_fwd(rep=0) == -1 and conv_fwd(rep=65) == -1 and conv_fwd(rep=-1) == -1
    assert conv_fwd(rep=8, q=A + 1024) == -1 and conv_fwd(rep=2, q=A + 256) == -1      # replicas: sumsq == sum + 64 doubles
    for f32 in (0, 1):
        assert conv_fwd(X=A + 8, f32=f32) == -3 and conv_fwd(W=A + 2, f32=f32) == -3 and conv_fwd(Y=A + 4, f32=f32) == -3
    assert conv_fwd(X=A + 8, s=None, q=None) == -3
    assert conv_fwd(X=None, Y=A + 4) == -1                                  # a null pointer is reported before a misaligned one


def conv_wgrad(dY=A, X=A, dWp=A, ws=None, ws_floats=0, n=3, Ti=6, Fi=32):
    return N.lib().audiossl_conv3x3_wgrad(dY, X, dWp, ws, ws_floats, n, Ti, Fi, None)


def test_conv_wgrad_rejects_bad_arguments():
    assert conv_wgrad(dY=None) == -1 and conv_wgrad(X=None) == -1 and conv_wgrad(dWp=None) == -1
    assert conv_wgrad(Fi=8) == -1 and conv_wgrad(Fi=64) == -1 and conv_wgrad(Fi=0) == -1
    assert conv_wgrad(n=0) == -1 and conv_wgrad(Ti=0) == -1
    assert conv_wgrad(X=A + 8) == -3 and conv_wgrad(dY=A + 2) == -3
    assert conv_wgrad(X=A + 8, ws=A, ws_floats=1 << 30) == -3


def test_pooled_bn_entries_reject_null_and_empty():
    lib = N.lib()
    assert lib.audiossl_bn_relu_pooled_fwd(1, None, A, A, A, 3, 3, 16, None) == -1
    assert lib.audiossl_bn_relu_pooled_fwd(1, A, A, A, None, 3, 3, 16, None) == -1
    assert lib.audiossl_bn_relu_pooled_fwd(1, A, None, A, A, 3, 3, 16, None) == -1
    assert lib.audiossl_bn_relu_pooled_fwd(2, A, A, A, A, 3, 3, 16, None) == -1
    assert lib.audiossl_bn_relu_pooled_fwd(1, A, A, A, A, 3, 0, 16, None) == -1

    def train(Praw=A, s=A, q=A + 512, rep=8, count=576.0, gamma=A, P=A, To=3):
        return lib.audiossl_bn_relu_pooled_train_fwd(1, Praw, s, q, rep, count, gamma, A, None, None, 0.1, 1e-5, P, A, A, A, A, 3, To, 16, None)
    assert train(Praw=None) == -1 and train(s=None) == -1 and train(gamma=None) == -1 and train(P=None) == -1
    assert train(count=0.0) == -1 and train(q=A + 1024) == -1 and train(rep=0) == -1 and train(To=0) == -1
