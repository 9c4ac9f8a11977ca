"""
Classes to support FASTA files: ``FastaFile`` and ``FastaReader`` of the reference's lib/bx/seq/fasta.py, with ``get`` answered on
the MI355X (bx.seq.seq.SeqFile: ``get_batch(starts, lengths)`` is the call to make).  A file is read as the reference reads it --
line by line up to the header that follows the wanted contig, which becomes ``lookahead`` -- so ``.name``, ``.length`` and ``.text``
are the reference's; whole files for the device are bxmi.sequence.TwoBitSet.from_fasta.
"""
from bx.seq.seq import SeqFile, SeqReader


class FastaFile(SeqFile):
    def __init__(self, file, revcomp=False, name="", gap=None, lookahead=None, contig=None, other="error"):
        SeqFile.__init__(self, file, revcomp, name, gap, other)
        self.lookahead = lookahead
        contig = 1 if contig is None else contig
        assert contig >= 1, f"contig {contig} is not legal"
        words, at = None, 1  # the wanted record's words so far (None: no line of any record yet); the record being read
        while True:
            if self.lookahead is not None:
                line, self.lookahead = self.lookahead, None
            else:
                line = self.file.readline()
                if not isinstance(line, str):
                    line = line.decode()
            if not line:
                break
            if line.startswith(">"):
                if words is not None:
                    if at == contig:
                        self.lookahead = line  # (the next record's header)
                        break
                    at += 1
                self.name = self.extract_name(line[1:])
                words = []
            elif words is None:
                words = line.split()  # (a headerless first record)
            else:
                words.extend(line.split())
        assert at == contig, f"contig {contig} is not legal (file contains only {at})"
        if words is not None:
            self.text = "".join(words)
            self.length = len(self.text)


class FastaReader(SeqReader):
    def __init__(self, file, revcomp=False, name="", gap=None):
        SeqReader.__init__(self, file, revcomp, name, gap)
        self.lookahead = None

    def __next__(self):
        seq = FastaFile(self.file, self.revcomp, self.name, self.gap, self.lookahead)
        if seq.text is None:
            return None
        self.lookahead = seq.lookahead
        self.seqs_read += 1
        return seq
