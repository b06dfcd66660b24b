"""SGZ_OPT_IMAGE_ONLY_SPLIT's range (sgz.h): 0, 1 and 2 .. 4096 frames per Nyquist workgroup are accepted, larger values refused --
the kernel divides the frame count by the value.  No GPU needed: the option is checked when it is set."""
import pytest

from signalizer_amd import api, config


@pytest.mark.parametrize("value", [0, 1, 2, 3, 8, 4096])
def test_accepted(value):
    plan = api.Plan(config.cfg2())
    plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, value)


@pytest.mark.parametrize("value", [4097, 1 << 20, 0xFFFFFFFF])
def test_refused(value):
    plan = api.Plan(config.cfg2())
    with pytest.raises(Exception):
        plan.set_option(api.OPT_IMAGE_ONLY_SPLIT, value)
