"""What the node-strain layers above the kernel refuse without a device: the CLI's --subset-strain, --strain-order and
--strain-min-nodes in every combination that is not a node field's strain (exit status 5 with a message, before any device is
touched), OpticalFlow.strain_options_ok, and the entry's workspace size."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ["a.raw", "b.raw", "96", "80", "t_"]  # (never opened: the options are judged first)
CHAIN = ["--correlation", "7", "--subset-refine", "7"]


def run_cli(args):
    exe = os.path.join(ROOT, "cuda-flow2d_amd", "host", "flow2d")
    return subprocess.run([exe] + args + TAIL, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,word", [
    (["--subset-strain", "2"], "--subset-refine"),                                   # no node field at all
    (["--subset-strain", "2", "--deformation"], "--subset-refine"),                  # the variational flow has no nodes
    (["--strain-order", "2"] + CHAIN, "belong to --subset-strain"),
    (["--strain-min-nodes", "5"] + CHAIN, "belong to --subset-strain"),
    (["--correlation", "7", "--subset-strain", "0"], "M >= 1"),                       # a search alone has no gradients
    (["--correlation-passes", "7:6:8", "--subset-strain", "0"], "M >= 1"),
    (CHAIN + ["--subset-strain", "0", "--strain-order", "2"], "window fit"),
    (CHAIN + ["--subset-strain", "8"], "0 .. 7"),
    (CHAIN + ["--subset-strain", "-1"], "0 .. 7"),
    (CHAIN + ["--subset-strain", "two"], "0 .. 7"),
    (CHAIN + ["--subset-strain"], "0 .. 7"),
    (CHAIN + ["--subset-strain", "2", "--strain-order", "3"], "1 .. 2"),
    (CHAIN + ["--subset-strain", "2", "--strain-order", "0"], "1 .. 2"),
    (CHAIN + ["--subset-strain", "2", "--strain-min-nodes", "2"], "least node count"),   # fewer than the fit's coefficients
    (CHAIN + ["--subset-strain", "2", "--strain-order", "2", "--strain-min-nodes", "5"], "least node count"),
    (CHAIN + ["--subset-strain", "1", "--strain-min-nodes", "10"], "least node count"),  # more than the window holds
    (CHAIN + ["--subset-strain", "2", "--strain-min-nodes", "-1"], "0 .. 225"),
    (CHAIN + ["--subset-strain", "2", "--strain", "large"], "small or green"),
])
def test_cli_refusals(flow2d, args, word):
    q = run_cli(args)
    assert q.returncode == 5, (args, q.stdout[-500:])
    assert word in q.stdout, (args, q.stdout[-500:])


def test_options_and_workspace_without_a_device(flow2d):
    ok = flow2d.OpticalFlow.strain_options_ok
    assert ok() and ok(0) and ok(0, 7, 99) and ok(7, 2, 225, 0, 1) and ok(1, 2, 9) and ok(2, 1, 3) and ok(2, 2, 0)
    for bad in ((8,), (-1,), (2, 0), (2, 3), (2, 1, 2), (2, 2, 5), (1, 1, 10), (2, 1, 0, 2), (2, 1, 0, -1), (2, 1, 0, 1, 2), (0, 1, 0, 1, -1)):
        assert not ok(*bad), bad
    need = flow2d.Context.node_strain_workspace_bytes
    assert need(0, 5) == need(5, 0) == need(5, 5, 0) == 0
    one = need(1, 1)
    assert one > 0 and one % 16 == 0
    # one slab per workgroup of 64 x 4 nodes and instance
    assert need(64, 4) == one and need(65, 4) == 2 * one and need(64, 5) == 2 * one and need(130, 21, 3) == 3 * 6 * 3 * one
