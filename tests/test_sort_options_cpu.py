"""bin/pipeline's checks of DRM_SAM_SORT, all of which run before the index or a device is touched (the directory holds
nothing but config.txt and two four-base FASTQ files): any value but unsorted and coordinate, coordinate without
use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1, and coordinate on a sparse index's header-only or DRM_SAM_L2_ROWS path
end the run with exit status 1 and a message that names the variable; unsorted passes the option checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = 'DRM_SAM_SORT must be unsorted or coordinate: '
NEEDS = ("DRM_SAM_SORT=coordinate needs use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1 and sequence queries: the keys are "
         "the lines' real RNAME and POS")
SPARSE = ("DRM_SAM_SORT=coordinate does not go with a sparse index's header-only SAM or DRM_SAM_L2_ROWS=1: those files "
          "are not written by the block loop")
CASES = [
    ("empty", "idx", {"DRM_SAM_SORT": ""}, {}, VALUES + '""'),
    ("queryname", "idx", {"DRM_SAM_SORT": "queryname"}, {}, VALUES + '"queryname"'),
    ("one", "idx", {"DRM_SAM_SORT": "1"}, {}, VALUES + '"1"'),
    ("capital", "idx", {"DRM_SAM_SORT": "Coordinate"}, {}, VALUES + '"Coordinate"'),
    ("bad_value_without_cigar", "idx", {"DRM_SAM_SORT": "x", "DRM_SAM_CIGAR": None}, {}, VALUES + '"x"'),
    ("no_cigar", "idx", {"DRM_SAM_SORT": "coordinate", "DRM_SAM_CIGAR": None}, {}, NEEDS),
    ("not_streaming", "idx", {"DRM_SAM_SORT": "coordinate"}, {9: "0"}, NEEDS),
    ("not_dynamic", "idx", {"DRM_SAM_SORT": "coordinate"}, {8: "0"}, NEEDS),
    ("header_only", "sparse", {"DRM_SAM_SORT": "coordinate"}, {}, SPARSE),
    ("l2_rows", "sparse", {"DRM_SAM_SORT": "coordinate", "DRM_SAM_L2_ROWS": "1"}, {}, SPARSE),
]


@pytest.fixture(scope="module")
def option_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_options")
    for name, stride in (("idx", 1), ("sparse", 4)):
        (d / name).mkdir()
        (d / name / "config.txt").write_text(f"ref_len: 150\nstride: {stride}\n")
    (d / "m1.fastq").write_text("@r0\nACGT\n+\nIIII\n@r1\nTTGA\n+\nIIII\n")
    return d


def _run(option_dir, prefix, env, argv):
    args = [os.path.join(ROOT, "bin", "pipeline"), prefix, "m1.fastq", "g.fna", "128", "4", "4", "out", "1", "1"]
    for i, v in argv.items():
        args[i] = v
    e = {k: v for k, v in os.environ.items() if not k.startswith("DRM_")}
    e.update({k: v for k, v in {"DRM_SAM_CIGAR": "1", **env}.items() if v is not None})
    return subprocess.run(args, cwd=option_dir, env=e, capture_output=True, text=True)


@pytest.mark.parametrize("prefix,env,argv,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_pipeline_rejects_bad_sort_options(option_dir, prefix, env, argv, message):
    r = _run(option_dir, prefix, env, argv)
    assert r.returncode == 1
    assert r.stderr == "Error: " + message + "\n"
    assert "Index loaded" not in r.stdout and not os.path.exists(option_dir / "out" / "results.sam")
    # the same run with a valid value ends later, where the directory cannot serve it, not at the option
    ok = _run(option_dir, "idx", {"DRM_SAM_SORT": "unsorted"}, {})
    assert ok.returncode == 1 and "DRM_SAM_SORT" not in ok.stderr and ok.stderr.startswith("Error: ")
