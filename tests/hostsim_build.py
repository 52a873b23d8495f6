"""The one compiler line of the host builds under tests/hostsim: a sim as a shared object for ctypes, or as a stand-alone program
(-DSIM_MAIN: the form the sanitizer builds take, run directly), with one set of warning flags."""
import os
import subprocess

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
WARN = ["-Wall", "-Wno-unused-function"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


class SimBuildError(RuntimeError):
    def __init__(self, cmd, stderr):
        super().__init__(" ".join(cmd) + "\n" + stderr[-4000:])
        self.stderr = stderr


def build_sim(sources, out, main=False, sanitize=False, extra=()):
    """Compile sources (names under tests/hostsim, paths, or objects) into `out`; returns out.  SimBuildError carries the compiler's words."""
    if isinstance(sources, str):
        sources = [sources]
    srcs = [s if os.path.isabs(s) else os.path.join(SIM_DIR, s) for s in sources]
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + WARN + (["-DSIM_MAIN"] if main else ["-fPIC", "-shared"]) + (SANITIZE if sanitize else [])
    cmd += list(extra) + ["-o", out] + srcs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SimBuildError(cmd, r.stderr)
    return out
