"""A plain Python port of klib's kseq_read and ks_getuntil2 (kseq.h): the parse that dashing's Encoder::for_each runs on
every input file, as the outside reference of the project's three FASTA/FASTQ parsers (the host FastxParser, the device
decoder kernels_fastx.hip, the CLI's raw staging).  It imports nothing from the project.

parse(data) -> (records, status): `records` is the list of (name, seq) -- both bytes -- that kseq_read returned before it
first returned a negative value, and `status` is that value (-1: end of file; -2: a FASTQ record without a quality
string or with one of another length).  dashing's encoder reads records while kseq_read >= 0, so the first error ends
the file and the record that caused it contributes nothing.  runs(seq) gives the maximal runs of ACGTacgt: all that the
k-mer encoder sees, for every k.

Which kseq: the reference tree's copy of klib is not at hand, so the version is unpinned; this follows current klib,
whose ks_getuntil2 drops one trailing '\\r' of a line read when the accumulated string is longer than one byte.  Old
klib without that strip would keep the '\\r' of every CRLF line end and split k-mers there; the project strips it, as
current klib does.  The project also drops a '\\r' that is a record's very first sequence byte (a first sequence line
of "\\r\\n"), which kseq keeps: that changes no ACGT run, so compare runs(), not bytes.
"""
import re

_SEP_SPACE, _SEP_LINE = 0, 2
_ISSPACE = frozenset(b" \t\n\v\f\r")
_RUN = re.compile(rb"[ACGTacgt]+")


class _Stream:
    def __init__(self, data):
        self.d = bytes(data)
        self.i = 0

    def getc(self):
        if self.i >= len(self.d):
            return -1
        c = self.d[self.i]
        self.i += 1
        return c

    def getuntil(self, sep, s, append):
        """ks_getuntil2: (length of s, the delimiter or 0); -1 when nothing at all was read (end of file)"""
        if not append:
            del s[:]
        d, b, n = self.d, self.i, len(self.d)
        if b >= n:  # !gotany && eof
            return -1, 0
        if sep == _SEP_LINE:
            i = d.find(b"\n", b)
            if i < 0:
                i = n
        else:
            i = b
            while i < n and d[i] not in _ISSPACE:
                i += 1
        s += d[b:i]
        dret = d[i] if i < n else 0
        self.i = i + 1 if i < n else n
        if sep == _SEP_LINE and len(s) > 1 and s[-1] == 0x0D:
            del s[-1]
        return len(s), dret


def _kseq_read(ks, st):
    """one kseq_read: (status, (name, seq) or None); st[0] is kseq's last_char"""
    if st[0] == 0:  # jump to the next header character, byte by byte
        while True:
            c = ks.getc()
            if c < 0:
                return c, None
            if c in (0x3E, 0x40):
                break
        st[0] = c
    name, comment, seq, qual = bytearray(), bytearray(), bytearray(), bytearray()
    r, c = ks.getuntil(_SEP_SPACE, name, False)
    if r < 0:
        return r, None
    if c != 0x0A:
        ks.getuntil(_SEP_LINE, comment, False)
    while True:
        c = ks.getc()
        if c < 0 or c in (0x3E, 0x2B, 0x40):
            break
        if c == 0x0A:
            continue
        seq.append(c)
        ks.getuntil(_SEP_LINE, seq, True)
    if c in (0x3E, 0x40):
        st[0] = c
    if c != 0x2B:  # FASTA
        return len(seq), (bytes(name), bytes(seq))
    while True:  # skip the rest of the '+' line
        c = ks.getc()
        if c < 0 or c == 0x0A:
            break
    if c == -1:
        return -2, None
    while True:
        r, _ = ks.getuntil(_SEP_LINE, qual, True)
        if not (r >= 0 and len(qual) < len(seq)):
            break
    st[0] = 0
    if len(seq) != len(qual):
        return -2, None
    return len(seq), (bytes(name), bytes(seq))


def parse(data):
    ks, st, records = _Stream(data), [0], []
    while True:
        r, rec = _kseq_read(ks, st)
        if r < 0:
            return records, r
        records.append(rec)


def runs(seq):
    """the maximal runs of ACGTacgt in seq, in order"""
    return _RUN.findall(bytes(seq))


def all_runs(records):
    """every record's runs, in record order (k-mers never span records)"""
    return [x for _, s in records for x in runs(s)]
