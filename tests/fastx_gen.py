"""FASTA / FASTQ text makers and the damage generator of the parse fuzz tests (tests/test_gpu_fastx.py on the device,
tests/test_host_parse_vs_kseq.py on the host).  Plain numpy; nothing from the project."""
import numpy as np


def fasta(rng, records, width, eol=b"\n", final_eol=True, blank_every=0):
    out = []
    for i, (name, seq) in enumerate(records):
        out.append(b">" + name + eol)
        s = bytes(seq)
        if width <= 0:
            out.append(s + eol)
        else:
            for x in range(0, len(s), width):
                out.append(s[x : x + width] + eol)
                if blank_every and (x // width) % blank_every == blank_every - 1:
                    out.append(eol)
    data = b"".join(out)
    if not final_eol and data.endswith(eol):
        data = data[: -len(eol)]
    return data


def fastq(rng, reads, eol=b"\n", final_eol=True, qual=None):
    out = []
    for i, r in enumerate(reads):
        q = qual(i, len(r)) if qual else bytes(rng.integers(33, 75, len(r), dtype=np.uint8))
        out.append(b"@read%d some text\n".replace(b"\n", eol) % i + bytes(r) + eol + b"+" + eol + q + eol)
    data = b"".join(out)
    if not final_eol and data.endswith(eol):
        data = data[: -len(eol)]
    return data


def random_text(rng, g):
    """a well-formed FASTA or FASTQ text over the sequence g: (data, eol)"""
    eol = b"\r\n" if rng.random() < 0.2 else b"\n"
    if rng.random() < 0.5:  # FASTA
        nrec = int(rng.integers(1, 6))
        cuts = sorted(set([0, len(g)] + [int(x) for x in rng.integers(0, len(g), nrec - 1)]))
        recs = [(bytes(rng.integers(33, 126, int(rng.integers(0, 90)), dtype=np.uint8)), g[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        data = fasta(rng, recs, int(rng.choice([0, 1, 7, 60, 63, 64, 65, 80, 200, 5000])), eol=eol, final_eol=bool(rng.random() < 0.7),
                     blank_every=int(rng.choice([0, 0, 3, 11])))
    else:  # FASTQ
        top = max(2, min(int(rng.choice([50, 300, 3000])), len(g) // 2))
        lens = [int(x) for x in rng.integers(1, top, int(rng.integers(1, 120)))]
        at, rds = 0, []
        for L in lens:
            rds.append(g[at : at + L])
            at = (at + L) % max(1, len(g) - top)
        data = fastq(rng, rds, eol=eol, final_eol=bool(rng.random() < 0.7))
    return data, eol


def damage(rng, data, eol):
    """lines dropped, doubled, cut, swapped, lengthened; '+' '@' '>' put at line starts; blank lines; single bytes overwritten
    (structure characters, NUL, high bytes, lone '\\r' / '\\n'); '\\r' and '\\r\\r\\n' anywhere -- headers, sequence and
    quality lines --; text before the first header and between records; empty reads; a cut on a '+' line"""
    lines = data.split(eol)
    for _ in range(int(rng.integers(1, 4))):
        if len(lines) < 2:
            break
        i = int(rng.integers(0, len(lines)))
        kind = int(rng.integers(0, 12))
        if kind == 0:
            del lines[i]
        elif kind == 1:
            lines.insert(i, lines[i])
        elif kind == 2:
            lines[i] = lines[i][: len(lines[i]) // 2]
        elif kind == 3:
            lines.insert(i, b"")
        elif kind == 4:
            lines[i] = bytes([int(rng.choice(list(b"+@>")))]) + lines[i]
        elif kind == 5 and i + 1 < len(lines):
            lines[i], lines[i + 1] = lines[i + 1], lines[i]
        elif kind == 6:
            lines[i] = lines[i] + bytes(rng.integers(33, 126, 5, dtype=np.uint8))
        elif kind == 7:  # a lone '\r' or '\r\r' inside a line (a header, a sequence or a quality line)
            at = int(rng.integers(0, len(lines[i]) + 1))
            lines[i] = lines[i][:at] + (b"\r" if rng.random() < 0.7 else b"\r\r") + lines[i][at:]
        elif kind == 8:  # text in front of a line: before the first header, behind a FASTQ record
            lines[i] = rng.choice(np.frombuffer(b"xACGT \t", np.uint8), int(rng.integers(1, 6))).tobytes() + lines[i]
        elif kind == 9:  # an empty read: header, empty sequence, '+', empty (or missing) quality
            lines[i:i] = [b"@empty", b"", b"+", b""] if rng.random() < 0.7 else [b"@empty", b"+"]
        elif kind == 10:  # quality (or sequence) a byte or two too long / too short
            lines[i] = lines[i] + b"I" * int(rng.integers(1, 3)) if rng.random() < 0.5 else lines[i][:-1]
        else:  # the text ends on a '+' line
            lines = lines[:i] + [b"+"]
    data = eol.join(lines)
    if rng.random() < 0.5 and len(data) > 4:
        buf = bytearray(data)
        for _ in range(int(rng.integers(1, 6))):
            buf[int(rng.integers(1, len(buf)))] = int(rng.choice(list(b"\n\r>@+\x00\xff NacgtACGT")))
        data = bytes(buf)
    if rng.random() < 0.2 and data:  # '\r\r\n' for one line end, or a '\r' at the very end
        if rng.random() < 0.5:
            at = data.find(b"\n", int(rng.integers(0, len(data))))
            if at >= 0:
                data = data[:at] + b"\r\r" + data[at:]
        else:
            data = data + b"\r"
    return data
