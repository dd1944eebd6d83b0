"""Read qualities on the GPU path: mirror of the quality model of the reference's src/quality/quality.rs.

The reference keeps a read's qualities remapped to eight classes (`remap_quality8`, quality.rs:33-43).  Here the quality line of
every kept read comes out of the ingest beside its bases (kmu_ingest_fastq_qual), kmu_quality_remap turns the bytes into classes
and kmu_read_qual_stats gives every read's class counts.  (The wavelet-matrix store and the ZMQ server are not mirrored.)
"""
import numpy as np

from . import _abi as A
from . import lib


def remap_quality8(q):
    """quality.rs:33-43 on a byte or an array of bytes, in integers: 0 below 0x25, then one class per three values, 7 from 0x37 on
    (the reference's f32 expression gives the same class for all 256 bytes)"""
    q = np.asarray(q, np.uint8).astype(np.int64)
    out = np.where(q < 0x25, 0, np.minimum(7, 1 + (q - 0x25) // 3)).astype(np.uint8)
    return out if out.ndim else int(out)


def quality_to_proba(q, qmin):
    """quality.rs:19-21: 10^((qmin - q) / 10); the reference subtracts in u8, so q above qmin is refused"""
    if int(q) > int(qmin):
        raise ValueError("quality_to_proba: q = %d above qmin = %d (the reference's u8 subtraction overflows)" % (q, qmin))
    return 10.0 ** ((int(qmin) - int(q)) / 10.0)


class QSequenceRaw:
    """quality.rs: the qualities of one read, one byte each -- here the classes of remap_quality8, as QSequenceWM::decompress
    gives them"""

    def __init__(self, read_num, qseq):
        self.read_num = int(read_num)
        self.qseq = np.asarray(qseq, np.uint8)

    def get_read_num(self):
        return self.read_num

    def __len__(self):
        return int(self.qseq.shape[0])


def load_quality_classes(text, ctx=None):
    """FASTQ text -> one QSequenceRaw per kept read (read_num: the read's rank among the records of the text), the classes
    computed on the device: ingest with qualities, then the remap in place"""
    from .sketching import default_context
    ctx = ctx or default_context()
    _, quals, offsets, _, index = ctx.ingest_fastq_qual(text, want_index=True)
    classes = ctx.quality_remap(quals, out=quals) if int(quals.shape[0]) else quals
    if lib._is_torch(classes):
        classes, offsets, index = classes.cpu().numpy(), offsets.cpu().numpy(), index.cpu().numpy()
    off = np.asarray(offsets).astype(np.int64)
    return [QSequenceRaw(int(index[i]) & 0xFFFFFFFF, classes[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def read_quality_stats(quals, offsets, ctx=None):
    """kmu_read_qual_stats: (records, class_hist) of the raw quality bytes of a batch -- records as a numpy array of
    A.READ_QUAL_DTYPE, class_hist uint64 [8] the bases of the batch per class"""
    from .sketching import default_context
    ctx = ctx or default_context()
    recs, hist = ctx.read_qual_stats(quals, offsets)
    if lib._is_torch(recs):
        recs = recs.cpu().numpy().view(np.dtype(A.READ_QUAL_DTYPE)).reshape(-1)
        hist = hist.cpu().numpy().view(np.uint64)
    return recs, hist
