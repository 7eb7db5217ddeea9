"""Writes tests/golden/data/minikeys.txt and tests/golden/ref_minikeys.json: the reference CLI's own
-m minikeys run (thread_process_minikeys, keyhunt.cpp:3094-3259) over two chunks.

Targets (tests/golden/data/minikeys.txt): the address of the reference's own tests/minikeys.txt (the
README's known answer SG64GZqySYwBm9KxE3wJ29, candidate 3000 from the base, valid ordinal 4), and the
address of SG64GZqySYwBm9KxETNxjq, the fifth valid candidate after the SECOND chunk's base
(candidate 730 from it, chosen with tests/_minikeys_model.py).  Chunk 2 starts 253 N candidates after
chunk 1 while chunk 1 walks about 256 N of them, so that candidate lies in both and the reference
records it twice: near the end of chunk 1 and at the start of chunk 2.

The run: oracle/_ref/keyhunt -m minikeys -f minikeys.txt -C SG64GZqySYwBm9KxE3wH8R -n 0x100000 -t 1
-M -s 0, one thread, stopped once its stdout holds the second "[+] Base minikey:" line and the hit
that follows it (a chunk is 2^20 valid minikeys, about 2.7e8 candidates: minutes on one core).
Recorded: argv, stdout up to and including that second line, and KEYFOUNDKEYFOUND.txt at the stop."""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
import _minikeys_model as M  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "keyhunt")
BASE = "SG64GZqySYwBm9KxE3wH8R"
KNOWN = "SG64GZqySYwBm9KxE3wJ29"
N = 0x100000
ARGV = ["-m", "minikeys", "-f", "minikeys.txt", "-C", BASE, "-n", hex(N), "-M"]
LINE = "[+] Base minikey: "


def overlap_minikey() -> str:
    second = M.advance(M.digits_of(BASE), N)
    return M.candidate(second, M.valid_offsets(second, 4096)[4])


def main(limit_s: int = 3600) -> None:
    targets = [M.record_of(KNOWN)["address"], M.record_of(overlap_minikey())["address"]]
    open(os.path.join(HERE, "data", "minikeys.txt"), "w").write("\n".join(targets) + "\n")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "minikeys.txt"), "w").write("\n".join(targets) + "\n")
        out_path = os.path.join(td, "stdout.txt")
        with open(out_path, "wb") as out:
            p = subprocess.Popen(["timeout", "-k", "10", str(limit_s), "stdbuf", "-o0", REF] + ARGV + ["-t", "1", "-s", "0"],
                                 cwd=td, stdout=out, stderr=subprocess.DEVNULL)
            try:
                while p.poll() is None:
                    time.sleep(2)
                    text = open(out_path, "rb").read().decode("latin-1")
                    second = text.find(LINE, text.find(LINE) + 1)
                    if second >= 0 and "HIT!!" in text[second:] and text.endswith("\n"):
                        break
            finally:
                p.terminate()
                p.wait()
        text = open(out_path, "rb").read().decode("latin-1")
        second = text.find(LINE, text.find(LINE) + 1)
        assert second >= 0, "the reference did not reach its second chunk in time"
        stdout = text[:text.index("\n", second) + 1]
        keyfound = open(os.path.join(td, "KEYFOUNDKEYFOUND.txt")).read()
    doc = {"_source": "tests/golden/make_minikeys_golden.py: the reference CLI, one thread, stopped in its second chunk",
           "argv": ARGV, "n": N, "base": BASE, "known": KNOWN, "overlap": overlap_minikey(),
           "stdout": stdout, "keyfound": keyfound}
    json.dump(doc, open(os.path.join(HERE, "ref_minikeys.json"), "w"), indent=1)
    print("wrote ref_minikeys.json:", len(stdout), "bytes of stdout,", keyfound.count("minikey: "), "records")


if __name__ == "__main__":
    main()
