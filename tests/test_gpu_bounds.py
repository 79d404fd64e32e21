"""Where the kernels write, on the device: every case of tests/bounds_cases.py on guarded device buffers
(tests/hipmem.py::GuardedBuffer) -- outputs of exactly the documented size between two guard bands of 1 MiB, poisoned before
the call; inputs checksummed; a second call into the dirty output; and the kernel each case was written for (kernel_used, the
kernel queries, the launch record).  No guard is expected to trip: one that does names the side, the offsets and the count."""
import pytest

from tests import bounds_cases as bc
from tests.hipmem import GuardedBuffer, guarded_for

pytestmark = pytest.mark.gpu


def test_the_checker_sees_one_byte_on_either_side_and_in_an_input(hip_lib):
    bc.checker_self_test(GuardedBuffer)


@pytest.mark.parametrize("name", bc.ids())
def test_kernels_write_inside_their_buffers(hip_lib, name):
    assert guarded_for(hip_lib) is GuardedBuffer
    bc.run(hip_lib, name)
