"""CPU: bench.py's command line.  A plain run is the headline alone; what takes runs of its
own is asked for with --full, and --dump-outputs names the folder of the last step's arrays."""

import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_parse():
    a = bench.parse(["--full", "--no-cpu", "--dump-outputs", "some/dir"])
    assert a.full is True and a.no_cpu is True and a.dump_outputs == "some/dir"
