"""lorahip_worker.h::ParkedThread -- the one thread-and-mailbox type behind the launch threads of the batch scheduler, the run threads
of a mixed level-3 handle and the helpers of the staging fills -- compiled for the HOST alone into a program of its own
(tests/worker_check.cpp) and run without a GPU. The program exits non-zero with a message on the first case that fails; its header
comment lists the cases' purpose and the sanitizer builds that are made by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lora_sdr_amd", "csrc")


def test_header_needs_nothing_but_the_standard_library():
    """a plain C++ program can include it: nothing from HIP, nothing from the project"""
    with open(os.path.join(CSRC, "lorahip_worker.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_round_trips_destruction_fan_out_and_post_all_wait_all(tmp_path):
    exe = str(tmp_path / "worker_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "worker_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "worker_check: ok"
