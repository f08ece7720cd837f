"""The two workspace size functions of the convolution backward are one plan: on the shared domain (stride 1, Cout == 16, Cin a
multiple of 16 up to 64) include/dtfill.h states dtfill_conv2d_wide_backward_workspace_bytes by reference to
dtfill_conv2d_backward_workspace_bytes, and the two must agree as integers.  Host arithmetic: no device."""
import pytest

FRAMES = ((1, 1, 1), (2, 33, 67), (3, 32, 64), (1, 64, 129))


@pytest.mark.parametrize("ksize", (1, 3, 5, 7))
@pytest.mark.parametrize("cin", (16, 32, 48, 64))
def test_the_narrow_and_the_wide_size_agree_on_the_shared_domain(pkg, ksize, cin):
    pkg.build()
    L = pkg.load()
    for B, H, W in FRAMES:
        narrow = L.dtfill_conv2d_backward_workspace_bytes(B, H, W, cin, ksize, 16)
        wide = L.dtfill_conv2d_wide_backward_workspace_bytes(B, H, W, cin, ksize, 16, 1, 0)
        assert narrow == wide and narrow > 0, (B, H, W, cin, ksize, narrow, wide)
    # no frames: both refuse
    assert L.dtfill_conv2d_backward_workspace_bytes(0, 33, 67, cin, ksize, 16) == 0
    assert L.dtfill_conv2d_wide_backward_workspace_bytes(0, 33, 67, cin, ksize, 16, 1, 0) == 0
