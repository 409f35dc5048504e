"""Device restatements of numpy's float32 routines, bit-for-bit (they are what makes the
TagContinuous float path bit-exact instead of 'within 1e-5')."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_device_math_is_numpy_exact():
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers import hip_driver as drv

    require_gpu()
    mod = drv.Module(drv.code_object_of("wd_test_math"))  # the test-only code object
    fn = mod.get_function("wd_test_math")
    rng = np.random.RandomState(0)
    n = 1 << 20
    from tests.test_oracle_golden import _tie_neighbourhoods

    ties = _tie_neighbourhoods()
    ties = ties[ties > 0]
    special = np.array([np.pi / 2, np.pi, 3 * np.pi / 2, 2 * np.pi, 6.2831855, 5 * np.pi / 4], np.float32)
    a = np.concatenate([(rng.rand(n - len(ties) - len(special)) * 2 * np.pi + 1e-3).astype(np.float32),
                        ties, special])
    b = (rng.rand(n) * 20 + 0.01).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(5)]
    fn(ta, tb, *outs, np.int32(n), block=(256, 1, 1), grid=(1024, 1))
    torch.cuda.synchronize()
    s, c, rem, sq, dv = (o.cpu().numpy() for o in outs)
    np.testing.assert_array_equal(s.view(np.uint32), np.sin(a).view(np.uint32))
    np.testing.assert_array_equal(c.view(np.uint32), np.cos(a).view(np.uint32))
    np.testing.assert_array_equal(rem.view(np.uint32), np.remainder(a, b).view(np.uint32))
    np.testing.assert_array_equal(sq.view(np.uint32), np.sqrt(a * a + b * b).view(np.uint32))
    np.testing.assert_array_equal(dv.view(np.uint32), (a / b).view(np.uint32))
    # negative dividends: numpy's remainder takes the divisor's sign
    a2 = (-a).astype(np.float32)
    fn(torch.from_numpy(a2).cuda(), tb, *outs, np.int32(n), block=(256, 1, 1), grid=(1024, 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs[2].cpu().numpy().view(np.uint32), np.remainder(a2, b).view(np.uint32))


def test_sincos_beyond_two_pi():
    """wd_np_sincosf where Acrobot and Pendulum call it: negative angles ([-2 pi, 2 pi]) and angles that are never wrapped
    (Pendulum's theta moves up to 0.4 rad per tick), up to the bound the routine's header states, |x| <= 71476.  2^20
    arguments: uniform on [-2 pi, 2 pi], uniform on +-[2 pi, 100], log-uniform on +-[100, 71476], +-k * float32(pi / 2)
    for k <= 64 and the negated tie neighbourhoods.  Sin and cos equal numpy's float32 kernels bit for bit (the contract of
    the test above), and lie within 1 float32 ulp of the float64 value rounded to float32 (which does not depend on the
    SIMD kernel the local numpy dispatches to: the Cody-Waite reduction and the two polynomials carry under 1 ulp)."""
    from tests.hip_harness import require_gpu, ulp_diff
    from tests.test_oracle_golden import _tie_neighbourhoods
    from warp_drive_amd.managers import hip_driver as drv

    require_gpu()
    fn = drv.Module(drv.code_object_of("wd_test_math")).get_function("wd_test_math")
    rng = np.random.RandomState(12)
    n = 1 << 20
    k = np.arange(0, 65, dtype=np.float32) * np.float32(np.pi / 2)
    ties = _tie_neighbourhoods()
    fixed = np.concatenate([k, -k, -ties[ties > 0], np.float32([71476.0, -71476.0, 100.0, -100.0])]).astype(np.float32)
    m = (n - len(fixed)) // 3
    sign = lambda size: rng.choice(np.float32([-1.0, 1.0]), size=size)
    a = np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, size=m).astype(np.float32),
                        rng.uniform(2 * np.pi, 100.0, size=m).astype(np.float32) * sign(m),
                        np.minimum(np.exp(rng.uniform(np.log(100.0), np.log(71476.0), size=n - len(fixed) - 2 * m)),
                                   71476.0).astype(np.float32) * sign(n - len(fixed) - 2 * m),
                        fixed])
    assert a.shape == (n,) and np.abs(a).max() == np.float32(71476.0)
    b = np.ones(n, np.float32)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(5)]
    fn(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), *outs, np.int32(n), block=(256, 1, 1), grid=(1024, 1))
    torch.cuda.synchronize()
    s, c = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    s64 = np.sin(a.astype(np.float64)).astype(np.float32)
    c64 = np.cos(a.astype(np.float64)).astype(np.float32)
    for name, got, np32, ref in (("sin", s, np.sin(a), s64), ("cos", c, np.cos(a), c64)):
        d = ulp_diff(got, ref)
        bad = got.view(np.uint32) != np32.view(np.uint32)
        first = float(np.abs(a[bad]).min()) if bad.any() else None
        print(f"wd_np_sincosf {name}: {int(bad.sum())} of {n} differ from numpy's float32 kernel (smallest |x| {first}), "
              f"{int((d > 0).sum())} 1 ulp from the rounded float64 value, largest {int(d.max())} ulp")
        reach = np.abs(a) <= 100.0  # Pendulum's reachable range first: a failure above it alone names the magnitude
        np.testing.assert_array_equal(got[reach].view(np.uint32), np32[reach].view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(got.view(np.uint32), np32.view(np.uint32), err_msg=name)
        assert d.max() <= 1, (name, int(d.max()), a[d > 1][:8])
