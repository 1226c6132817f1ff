"""tests/kseq_ref.py, the kseq port every parse test takes its expectation from, pinned on hand-written cases whose
expected records were worked out by hand from klib's kseq_read / ks_getuntil2."""
import pytest

from kseq_ref import all_runs, parse, runs  # (tests/kseq_ref.py)

# (input, expected records, expected final status)
CASES = [
    # the issue's table
    (b">a\nACGTAC\rGTACGT\n", [(b"a", b"ACGTAC\rGTACGT")], -1),
    (b">a\nACGTAC\r\r\nGTACGT\n", [(b"a", b"ACGTAC\rGTACGT")], -1),
    (b"xx>a\nACGT\n", [(b"a", b"ACGT")], -1),
    (b"@a\nAC\rGT\n+\nIIIII\n", [(b"a", b"AC\rGT")], -1),
    (b"@a\nACGT\n+\nII\rII\n@b\nGGGG\n+\nIIII\n", [], -2),
    (b"@a\n+\n@b\nGGGG\n+\nIIII\n", [], -2),
    (b"@a\nACGT\n+", [], -2),
    # CRLF: the '\r' of every line end goes (the accumulated string is longer than one byte)
    (b">r1 desc\r\nACGT\r\nGGCC\r\n>r2\r\nTTTT\r\n", [(b"r1", b"ACGTGGCC"), (b"r2", b"TTTT")], -1),
    (b"@q\r\nACGT\r\n+\r\nIIII\r\n", [(b"q", b"ACGT")], -1),
    # ... but not when it is the only byte so far: a first sequence line "\r\n" keeps it
    (b">a\r\n\r\nACGT\r\n", [(b"a", b"\rACGT")], -1),
    # a first quality line "\r" counts one byte: record a fails, b is never read
    (b"@a\n\n+\n\r\n@b\nACGT\n+\nIIII\n", [], -2),
    (b"@a\n\r\n+\n\r\n", [(b"a", b"\r")], -1),
    # blank lines are skipped in sequence, read as (empty) quality lines
    (b">a\n\nACGT\n\n\nGG\n\n>b\n", [(b"a", b"ACGTGG"), (b"b", b"")], -1),
    (b"@a\nACGT\n+\n\nII\n\nII\n", [(b"a", b"ACGT")], -1),
    # '>' inside a line is a sequence byte; at a line start it begins a record
    (b">a\nAC>GT\n>b c>d\nTT\n", [(b"a", b"AC>GT"), (b"b", b"TT")], -1),
    # tab-separated and empty names; the name ends at the first white space
    (b">id1\tsome thing\nAC\n>\nGG\n> x\nTT\n>\x0bv\nA\n", [(b"id1", b"AC"), (b"", b"GG"), (b"", b"TT"), (b"", b"A")], -1),
    (b">a\rb c\nACGT\n", [(b"a", b"ACGT")], -1),
    # multi-line FASTQ; quality lines that begin with '@' '+' '>'
    (b"@q1\nACGT\nAC\n+q1\n@@+\n>@@\n@q2\nG\n+\n+\n", [(b"q1", b"ACGTAC"), (b"q2", b"G")], -1),
    # empty reads with an empty quality line; text after a FASTQ record is skipped up to the next '>' / '@'
    (b"@e\n+\n\n@f\nAC\n+\nII\njunk AC @g\nTT\n+\nII\n", [(b"e", b""), (b"f", b"AC"), (b"g", b"TT")], -1),
    # quality too long (one line) / too short at the end of the file
    (b"@a\nAC\n+\nIII\n", [], -2),
    (b"@a\nAC\n+\nII\n@b\nACGT\n+\nII\n", [(b"a", b"AC")], -2),
    # no final newline
    (b">a\nACGT", [(b"a", b"ACGT")], -1),
    (b">a\nACGT\r", [(b"a", b"ACGT")], -1),
    (b">a\nACGT\n\r", [(b"a", b"ACGT\r")], -1),  # a '\r' read as the first byte of a line at EOF: nothing follows, it stays
    (b"@a\nACGT\n+\nIIII", [(b"a", b"ACGT")], -1),
    (b"@a\nACGT\n+\nIIII\r", [(b"a", b"ACGT")], -1),
    # a lone '>' at the end is no record; '>a' at the end is an empty one
    (b">a\nAC\n>", [(b"a", b"AC")], -1),
    (b">a\nAC\n>b", [(b"a", b"AC"), (b"b", b"")], -1),
    # a '+' line in a '>' file starts a quality string
    (b">a\nACGT\n+\nIIII\n>b\nGG\n", [(b"a", b"ACGT"), (b"b", b"GG")], -1),
    # a FASTQ record without '+' at the end of the file is a FASTA record
    (b"@a\nAC\n+\nII\n@b\nGGTT\n", [(b"a", b"AC"), (b"b", b"GGTT")], -1),
    # an empty line strips a '\r' an earlier quality line left behind
    (b"@a\nACGT\n+\nI\r\r\n\nIII\n", [(b"a", b"ACGT")], -1),
    (b"", [], -1),
    (b"no header at all\n", [], -1),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_hand_cases(i):
    data, want, status = CASES[i]
    recs, st = parse(data)
    assert recs == want, (data, recs)
    assert st == status


def test_runs():
    assert runs(b"ACGTAC\rGTACGT") == [b"ACGTAC", b"GTACGT"]
    assert runs(b"NNacgtNxAC") == [b"acgt", b"AC"]
    assert runs(b"") == [] and runs(b"\r") == []
    assert all_runs([(b"a", b"ACNGT"), (b"b", b"TT")]) == [b"AC", b"GT", b"TT"]
