"""The table the defaults of history rectification are taken from (docs/LOG.md, "History rectification").  usage (GPU box): python tools/rectify_quality.py

tests/test_gpu_rectify.py's sequence -- cornell_blocks at 128 x 128, a still camera, 16 frames at one sample with the short block at rest, then 12 with it
translated -- for radius 1 ... 3, k 1 / 2 / 3, SHORTEN on and off and fast histories of 4 and 8 frames: rms error against 1024 samples of the new pose at 1, 2, 4,
8 and 12 frames after the step, over the static pixels whose light changed / did not.  Prints one JSON object."""
import json
import sys

sys.path.insert(0, ".")


def main():
    from tests.test_gpu_rectify import quality_sequence

    configs = {f"r{r}_k{k}_{'shorten' if s else 'keep'}_fast{n}": (r, float(k), s, float(n)) for r in (1, 2, 3) for k in (1, 2, 3) for s in (True, False) for n in (4, 8)}
    q = quality_sequence(configs)
    for table in ("rms", "clamped"):
        q[table] = {name: {str(f): [round(v, 5) for v in pair] for f, pair in rows.items()} for name, rows in q[table].items()}
    print(json.dumps(q))


if __name__ == "__main__":
    main()
