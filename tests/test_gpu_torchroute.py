"""The shared spin measurement of the device-route cases (tests/torchroute.py) can fail: tests/torchroute_cases.py in a child process."""
import pytest

from routecheck import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["the_spin_measurement_tells_a_call_that_waits"])
def test_torch_route(case):
    run_case("torchroute_cases", case)
