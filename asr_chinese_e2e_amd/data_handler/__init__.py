from .vocab import Vocab
from .padder import Padder
from .batch import collat, synthetic_pack, DataConfigAiShell1
from .processor import AudioParser, build_LFR_features
from .loader import BatchPlan, BucketedWaveLoader, WaveDataset, bucket_batches, build_dataloader, load_wav, shard_batches
from . import speed
from . import noise
from .noise import NoiseBank, RirBank
from . import specaug
from .specaug import SpecAugmentPolicy
from . import cmvn
from .cmvn import CmvnAccumulator, load_cmvn, load_cmvn_meta, save_cmvn, save_wenet_cmvn
from .stream_frontend import StreamingFrontEnd
